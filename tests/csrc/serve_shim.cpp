// serve_shim.cpp — the serve-plan arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_serve_device.h) compiled for the host, as
// dr_shim.cpp does for reset-time randomisation.  TEST INFRASTRUCTURE ONLY.  Built by tests/serve_shim_binding.py with -ffp-contract=off,
// the switch ppenv_serve.hip is compiled with.  plan->cells is a host pointer here.
#include "../../isaacgym_amd/csrc/ppenv_serve_device.h"

extern "C" {

size_t serve_shim_sizeof_plan() { return sizeof(pp_serve_plan); }
size_t serve_shim_sizeof_cell() { return sizeof(pp_serve_cell); }

// pp_serve_plan_upload's validator: 0, or the rule that is broken
int serve_shim_invalid(const pp_serve_plan* plan, const pp_serve_cell* cells) { return pp::serve_plan_invalid(*plan, cells); }

// pp_serve_fill on host memory
void serve_shim_fill(const pp_serve_plan* plan, float* out, const uint32_t* count) {
    for (int32_t e = 0; e < plan->num_envs; ++e) pp::serve_fill_env(*plan, e, out, count);
}

// pp_serve_apply on host memory: what serve_apply_kernel's lanes do, env by env
void serve_shim_apply(const pp_serve_plan* plan, const int64_t* reset_buf, float* out, uint32_t* count) {
    for (int32_t e = 0; e < plan->num_envs; ++e) pp::serve_step_env(*plan, e, reset_buf, out, count);
}

// pp_serve_apply_ids on host memory
void serve_shim_apply_ids(const pp_serve_plan* plan, const int64_t* env_ids, int32_t m, float* out, uint32_t* count) {
    for (int32_t i = 0; i < m; ++i)
        if (env_ids[i] >= 0 && env_ids[i] < plan->num_envs) pp::serve_advance_env(*plan, (int32_t)env_ids[i], out, count);
}

// the velocity of three draws as this unit instantiates serve_from_draws
void serve_shim_velocity(int32_t form, float speed, float tilt_deg, float tilt_z_deg, float* v) {
    const pp::V3 r = pp::serve_from_draws(form, speed, tilt_deg, tilt_z_deg);
    v[0] = r.x; v[1] = r.y; v[2] = r.z;
}

}
