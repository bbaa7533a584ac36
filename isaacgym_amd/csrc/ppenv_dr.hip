// ppenv_dr.hip — reset-time, per-env domain randomisation on the device (include/ppenv_dr.h).
//
// A streaming kernel: one lane per env, the row loop inside the lane, so the lanes of a wave store consecutive floats of one table row.
// The reset mask leaves most lanes idle on most steps: such a lane reads reset_buf[e], reads and writes randomize_buf[e], and is done.
// The plan is read-only device memory (wave-uniform: scalar loads); the per-env arithmetic is ppenv_dr_device.h.
//
// Shared scalars.  The control-step count (schedules; count == 0 is the first-application flag) is read by every lane and advanced by
// the launch itself, so that a captured launch replays correctly.  Each workgroup owns a copy, steps[blockIdx.x]: every lane loads it,
// the workgroup meets at __syncthreads(), then lane 0 stores count + 1.  No other workgroup ever touches that word, and within the
// workgroup the barrier orders all loads before the store — nothing a workgroup reads in a launch is rewritten in that launch by
// anyone but itself, after it has read it.  randomize_buf[e], draws[e] and column e of the tables belong to lane e alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_dr_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = PPENV_DR_BLOCK;

inline int32_t blocks_of(int32_t n) { return (n + kBlock - 1) / kBlock; }

__global__ __launch_bounds__(kBlock) void dr_apply_kernel(const ppenv_dr_plan* __restrict__ plan, const int64_t* __restrict__ reset_buf,
                                                          int64_t* __restrict__ randomize_buf, int64_t* __restrict__ steps,
                                                          int32_t* __restrict__ draws, int32_t n_state) {
    // Bounds come from the kernel argument (the size the state block and randomize_buf were made for), not from the plan: the loads of
    // steps[], randomize_buf[e] and the plan's scalars are then independent and leave together — an idle lane waits for two memory round
    // trips (those, then reset_buf[rows * e]) instead of four in a chain.  The plan's own num_envs bounds the table columns.
    if ((int64_t)blockIdx.x * kBlock >= n_state) return;
    const int64_t count = steps[blockIdx.x];
    const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const bool live = e < n_state;
    int64_t rnd = live ? randomize_buf[e] : 0;
    const int32_t rows = plan->reset_rows, frequency = plan->frequency;
    __syncthreads();                                           // every lane of this workgroup holds `count` before it is rewritten
    if (threadIdx.x == 0) steps[blockIdx.x] = count + 1;
    if (!live) return;
    const bool fire = pp::dr_step_rule(count == 0, reset_buf[(size_t)rows * (size_t)e], frequency, rnd);
    randomize_buf[e] = rnd;
    if (!fire || e >= plan->num_envs) return;
    pp::dr_redraw_env(*plan, e, count + 1, draws);
}

__global__ __launch_bounds__(kBlock) void dr_apply_ids_kernel(const ppenv_dr_plan* __restrict__ plan, const int64_t* __restrict__ env_ids, int32_t m,
                                                              int64_t* __restrict__ randomize_buf, const int64_t* __restrict__ steps,
                                                              int32_t* __restrict__ draws, int32_t n_state) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= m) return;
    const int32_t n = min(plan->num_envs, n_state);            // (a rare, host-driven path: the chain of loads does not matter here)
    const int64_t id = env_ids[i];
    if (id < 0 || id >= n) return;
    const int32_t e = (int32_t)id;
    const int64_t count = steps[e / kBlock];                   // read-only in this launch
    pp::dr_ids_env(*plan, e, count, randomize_buf, draws);
}

}  // namespace

extern "C" size_t ppenv_dr_state_draws_offset(int32_t num_envs) {
    return num_envs > 0 ? (size_t)blocks_of(num_envs) * sizeof(int64_t) : 0;
}

extern "C" size_t ppenv_dr_state_bytes(int32_t num_envs) {
    return num_envs > 0 ? ppenv_dr_state_draws_offset(num_envs) + (size_t)num_envs * sizeof(int32_t) : 0;
}

extern "C" int ppenv_dr_plan_upload(const ppenv_dr_plan* p, ppenv_dr_plan* plan_dev, void* stream) {
    bool ok = p && plan_dev && p->num_envs > 0 && p->env_id_offset >= 0 && p->frequency >= 1 && (p->reset_rows == 1 || p->reset_rows == 2) &&
              p->num_tables >= 1 && p->num_tables <= PPENV_DR_MAX_TABLES;
    for (int i = 0; ok && i < p->num_tables; ++i) {
        const ppenv_dr_entry& en = p->entry[i];
        ok = en.table && en.rows >= 1 && en.rows <= PPENV_DR_MAX_ROWS &&
             (en.distribution == PPENV_DR_UNIFORM || en.distribution == PPENV_DR_GAUSSIAN) &&
             (en.operation == PPENV_DR_SCALING || en.operation == PPENV_DR_ADDITIVE) &&
             (en.schedule == PPENV_DR_SCHED_NONE || (en.schedule == PPENV_DR_SCHED_LINEAR && en.schedule_steps > 0) ||
              (en.schedule == PPENV_DR_SCHED_CONSTANT && en.schedule_steps >= 0));
    }
    if (!ok) {
        ppenv_set_error("ppenv_dr_plan_upload: NULL pointer, num_envs <= 0, frequency < 1, reset_rows not 1 or 2, not 1..8 tables, or an entry with a "
                        "NULL table, rows outside 1..64, an unknown distribution / operation / schedule or a schedule without its schedule_steps");
        return PPENV_EINVAL;
    }
    if (hipMemcpyAsync(plan_dev, p, sizeof(ppenv_dr_plan), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {                    // set-up, once: *p may live on the caller's stack
        (void)hipGetLastError();
        ppenv_set_error("ppenv_dr_plan_upload: copying the plan to the device failed");
        return PPENV_EHIP;
    }
    return PPENV_OK;
}

extern "C" int ppenv_dr_apply(const ppenv_dr_plan* plan_dev, int32_t num_envs, const int64_t* reset_buf, int64_t* randomize_buf, void* state_dev,
                              void* stream) {
    if (!plan_dev || !reset_buf || !randomize_buf || !state_dev || num_envs <= 0) {
        ppenv_set_error("ppenv_dr_apply: NULL pointer or num_envs <= 0");
        return PPENV_EINVAL;
    }
    int64_t* steps = (int64_t*)state_dev;
    int32_t* draws = (int32_t*)((char*)state_dev + ppenv_dr_state_draws_offset(num_envs));
    hipLaunchKernelGGL(dr_apply_kernel, dim3(blocks_of(num_envs)), dim3(kBlock), 0, (hipStream_t)stream, plan_dev, reset_buf, randomize_buf, steps, draws, num_envs);
    return pp_launched("launching dr_apply_kernel failed");
}

extern "C" int ppenv_dr_apply_ids(const ppenv_dr_plan* plan_dev, int32_t num_envs, const int64_t* env_ids, int32_t count, int64_t* randomize_buf,
                                  void* state_dev, void* stream) {
    if (!plan_dev || !randomize_buf || !state_dev || num_envs <= 0 || count < 0 || (count > 0 && !env_ids)) {
        ppenv_set_error("ppenv_dr_apply_ids: NULL pointer, num_envs <= 0 or count < 0");
        return PPENV_EINVAL;
    }
    if (count == 0) return PPENV_OK;
    const int64_t* steps = (const int64_t*)state_dev;
    int32_t* draws = (int32_t*)((char*)state_dev + ppenv_dr_state_draws_offset(num_envs));
    hipLaunchKernelGGL(dr_apply_ids_kernel, dim3(blocks_of(count)), dim3(kBlock), 0, (hipStream_t)stream, plan_dev, env_ids, count, randomize_buf, steps, draws, num_envs);
    return pp_launched("launching dr_apply_ids_kernel failed");
}
