// dr_shim.cpp — the reset-time domain-randomisation arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_dr_device.h) compiled
// for the host, as host_shim.cpp does for the step.  TEST INFRASTRUCTURE ONLY.  Built by tests/dr_shim_binding.py with
// -ffp-contract=off: the header's products and sums round one by one, its fused ones are explicit fmaf() calls.
#include "../../isaacgym_amd/csrc/ppenv_dr_device.h"

extern "C" {

// the salted counter-RNG uniform of key k (what dr_base feeds on)
float dr_shim_uniform(uint64_t seed, uint32_t gid, uint32_t draw, uint32_t k) { return pp::rng_uniform(seed ^ PPENV_DR_SEED_SALT, gid, draw, k); }

// U[0,1) or the unit normal of key k
float dr_shim_base(uint64_t seed, uint32_t gid, uint32_t draw, uint32_t k, int32_t distribution) { return pp::dr_base(seed, gid, draw, k, distribution); }

float dr_shim_weight(int32_t schedule, int32_t schedule_steps, int64_t t) { return pp::dr_schedule_weight(schedule, schedule_steps, t); }

float dr_shim_value(const ppenv_dr_entry* en, uint64_t seed, uint32_t gid, uint32_t draw, uint32_t k, int64_t t) {
    return pp::dr_value(*en, seed, gid, draw, k, t);
}

// ppenv_dr_apply on host memory: what dr_apply_kernel's lanes do, env by env.  *count is the one control-step count (the device keeps
// an equal copy per workgroup).
void dr_shim_apply(const ppenv_dr_plan* plan, const int64_t* reset_buf, int64_t* randomize_buf, int64_t* count, int32_t* draws) {
    for (int32_t e = 0; e < plan->num_envs; ++e) pp::dr_step_env(*plan, e, *count, reset_buf, randomize_buf, draws);
    *count += 1;
}

// ppenv_dr_apply_ids on host memory
void dr_shim_apply_ids(const ppenv_dr_plan* plan, const int64_t* env_ids, int32_t m, int64_t* randomize_buf, const int64_t* count, int32_t* draws) {
    for (int32_t i = 0; i < m; ++i)
        if (env_ids[i] >= 0 && env_ids[i] < plan->num_envs) pp::dr_ids_env(*plan, (int32_t)env_ids[i], *count, randomize_buf, draws);
}

}
