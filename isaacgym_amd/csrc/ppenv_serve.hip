// ppenv_serve.hip — the serve plan on the device (include/ppenv_serve.h): each env's next serve, kept in the override buffer its step reads.
//
// Streaming kernels in the shape of ppenv_dr.hip: one lane per env, PP_SERVE_BLOCK envs per workgroup, the ragged tail guarded.  The reset
// mask leaves most lanes idle on most steps: such a lane reads reset_buf[rows * e] (coalesced) and is done.  A resetting lane reads and
// writes count[e] and stores its serve: layout 0 as one float per component row (consecutive lanes, consecutive floats), layout 1 as its
// own 20-byte row, unstaged — a handful of lanes per launch write one.  The plan and its cells are read-only device memory; the per-env
// arithmetic is ppenv_serve_device.h.  count[e] and env e's part of `out` belong to lane e alone: no shared word, no barrier, no atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_serve_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = PP_SERVE_BLOCK;

inline int32_t blocks_of(int32_t n) { return (n + kBlock - 1) / kBlock; }

__global__ __launch_bounds__(kBlock) void serve_fill_kernel(const pp_serve_plan* __restrict__ plan, int32_t n_arg, float* __restrict__ out,
                                                            const uint32_t* __restrict__ count) {
    const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (e >= n_arg || e >= plan->num_envs) return;
    pp::serve_fill_env(*plan, e, out, count);
}

__global__ __launch_bounds__(kBlock) void serve_apply_kernel(const pp_serve_plan* __restrict__ plan, int32_t n_arg, const int64_t* __restrict__ reset_buf,
                                                             float* __restrict__ out, uint32_t* __restrict__ count) {
    // the grid's bound is the kernel argument, so the reset_buf load waits only for the plan's reset_rows (a scalar load), not for two in a chain
    const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (e >= n_arg) return;
    if (reset_buf[(size_t)plan->reset_rows * (size_t)e] == 0 || e >= plan->num_envs) return;
    pp::serve_advance_env(*plan, e, out, count);
}

__global__ __launch_bounds__(kBlock) void serve_apply_ids_kernel(const pp_serve_plan* __restrict__ plan, int32_t n_arg, const int64_t* __restrict__ env_ids,
                                                                 int32_t m, float* __restrict__ out, uint32_t* __restrict__ count) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= m) return;
    const int64_t id = env_ids[i];
    if (id < 0 || id >= (int64_t)min(n_arg, plan->num_envs)) return;
    pp::serve_advance_env(*plan, (int32_t)id, out, count);
}

}  // namespace

extern "C" int pp_serve_plan_upload(const pp_serve_plan* p, const pp_serve_cell* cells, pp_serve_plan* plan_dev, pp_serve_cell* cells_dev, void* stream) {
    if (!p || !cells || !plan_dev || !cells_dev) {
        ppenv_set_error("pp_serve_plan_upload: NULL pointer");
        return PPENV_EINVAL;
    }
    if (const int why = pp::serve_plan_invalid(*p, cells)) {
        static const char* const text[] = {"", "groups * envs_per_group != num_envs, or one of them < 1", "env_id_offset < 0 or paired not 0 / 1",
                                           "unknown form (a PPENV_VARIANT_* value)", "unknown layout", "reset_rows not 1 or 2",
                                           "a cell with a non-finite value or lo > hi", "a tilt or tilt_z bound beyond +-57 degrees (the short sine / cosine series)"};
        pp_set_errorf("pp_serve_plan_upload: %s", text[why]);
        return PPENV_EINVAL;
    }
    pp_serve_plan host = *p;
    host.cells = cells_dev;
    if (hipMemcpyAsync(cells_dev, cells, (size_t)p->groups * sizeof(pp_serve_cell), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipMemcpyAsync(plan_dev, &host, sizeof(pp_serve_plan), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {                    // set-up, once: `host` lives on this stack
        (void)hipGetLastError();
        ppenv_set_error("pp_serve_plan_upload: copying the plan to the device failed");
        return PPENV_EHIP;
    }
    return PPENV_OK;
}

extern "C" int pp_serve_fill(const pp_serve_plan* plan_dev, int32_t num_envs, float* out, const uint32_t* count, void* stream) {
    if (!plan_dev || !out || !count || num_envs <= 0) {
        ppenv_set_error("pp_serve_fill: NULL pointer or num_envs <= 0");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(serve_fill_kernel, dim3(blocks_of(num_envs)), dim3(kBlock), 0, (hipStream_t)stream, plan_dev, num_envs, out, count);
    return pp_launched("launching serve_fill_kernel failed");
}

extern "C" int pp_serve_apply(const pp_serve_plan* plan_dev, int32_t num_envs, const int64_t* reset_buf, float* out, uint32_t* count, void* stream) {
    if (!plan_dev || !reset_buf || !out || !count || num_envs <= 0) {
        ppenv_set_error("pp_serve_apply: NULL pointer or num_envs <= 0");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(serve_apply_kernel, dim3(blocks_of(num_envs)), dim3(kBlock), 0, (hipStream_t)stream, plan_dev, num_envs, reset_buf, out, count);
    return pp_launched("launching serve_apply_kernel failed");
}

extern "C" int pp_serve_apply_ids(const pp_serve_plan* plan_dev, int32_t num_envs, const int64_t* env_ids, int32_t n_ids, float* out, uint32_t* count,
                                  void* stream) {
    if (!plan_dev || !out || !count || num_envs <= 0 || n_ids < 0 || (n_ids > 0 && !env_ids)) {
        ppenv_set_error("pp_serve_apply_ids: NULL pointer, num_envs <= 0 or n_ids < 0");
        return PPENV_EINVAL;
    }
    if (n_ids == 0) return PPENV_OK;
    hipLaunchKernelGGL(serve_apply_ids_kernel, dim3(blocks_of(n_ids)), dim3(kBlock), 0, (hipStream_t)stream, plan_dev, num_envs, env_ids, n_ids, out, count);
    return pp_launched("launching serve_apply_ids_kernel failed");
}
