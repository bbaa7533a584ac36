// ppenv_dr_adr.hip — automatic domain randomisation on the device (include/ppenv_dr_adr.h): a current range per randomised table, a share
// of the envs pinned to one boundary of one table for a whole game, each finished game credited to its boundary, each boundary moved
// outward or back in once per epoch by the mean return of its games.
//
// The reference has no ADR: the rule is this project's own specification (the header states it), unpinned by any oracle.
//
// fill / step are streaming kernels in the shape of ppenv_dr.hip: one lane per env, PPENV_DR_BLOCK envs per workgroup, the ragged tail
// guarded, the row loop inside the lane so that the lanes of a wave store consecutive floats of one table row.  The struct is read-only
// device memory (wave-uniform: scalar loads); every store is a plain vector store.  Every per-env word (draws, slot, ret, column e of the
// tables, the env's staging entries) belongs to lane e alone.  range[] is read-only in the step; the fill's workgroup 0 writes it and
// draws from the same values computed from the struct, not read; the update is one workgroup.  So no word is read by one workgroup and
// written by another in one launch.
//
// A step's idle lane.  The bound is the kernel argument (the size the state was made for), not the struct's num_envs, so the loads of
// ret[e] and of the struct's reset_rows / num_agents are independent and leave together; rew[A e] and reset[rows e] follow: two dependent
// memory round trips, as dr_apply_kernel arranges, then the stores of ret[e] and fin_slot_t[e].  The struct's num_envs bounds the table
// columns on the rare path that redraws.
//
// update: one workgroup, lane s per slot (17 at most).  A slot's words — its accumulators, its mean, and for a boundary slot range[s] —
// are that lane's alone: no barrier, no LDS.
//
// The fold is pp_serve_curric_fold (ppenv_serve_curric.hip), which is generic over (bin, q) pairs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_dr_adr_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = PPENV_DR_BLOCK;
static_assert(kBlock >= PP_ADR_MAX_SLOTS, "one lane per slot: the fill's first workgroup, the update");

__global__ __launch_bounds__(kBlock) void adr_fill_kernel(const pp_dr_adr* __restrict__ A, int32_t n_arg, int32_t d_arg, pp_dr_adr_state S) {
    const int32_t D = min(d_arg, A->dims);
    if (blockIdx.x == 0 && (int32_t)threadIdx.x < 2 * D)
        S.range[threadIdx.x] = pp::AdrStarts{}(*A, (int32_t)threadIdx.x >> 1, (int32_t)threadIdx.x & 1);
    const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (e >= n_arg || e >= A->num_envs) return;
    pp::adr_fill_env(*A, D, e, S);
}

__global__ __launch_bounds__(kBlock) void adr_step_kernel(const pp_dr_adr* __restrict__ A, int32_t n_arg, const float* __restrict__ rew,
                                                          const int64_t* __restrict__ reset, pp_dr_adr_state S, int32_t* __restrict__ fin_slot_t,
                                                          int64_t* __restrict__ fin_q_t) {
    const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (e >= n_arg) return;
    pp::adr_step_env(*A, e, rew, reset, S, fin_slot_t, fin_q_t);
}

__global__ __launch_bounds__(kBlock) void adr_update_kernel(const pp_dr_adr* __restrict__ A, int32_t d_arg, const int64_t* __restrict__ tot, pp_dr_adr_state S) {
    const int32_t D = min(d_arg, A->dims), s = (int32_t)threadIdx.x;
    if (s < 2 * D + 1) pp::adr_update_slot(*A, D, s, tot, S);
}

bool state_ok(const pp_dr_adr_state* s) {
    return s && s->range && s->draws && s->slot && s->ret && s->acc_n && s->acc_q && s->games && s->dropped && s->mean && s->widened && s->narrowed;
}

}  // namespace

extern "C" int pp_dr_adr_upload(const pp_dr_adr* a, double boundary_frac, pp_dr_adr* adr_dev, void* stream) {
    if (!a || !adr_dev) {
        ppenv_set_error("pp_dr_adr_upload: NULL pointer");
        return PPENV_EINVAL;
    }
    int32_t which = -1;
    if (const int why = pp::adr_invalid(*a, boundary_frac, &which)) {
        static const char* const text[] = {"", "num_envs < 1", "env_id_offset < 0", "reset_rows not 1 or 2", "num_agents not 1 or 2", "dims outside 1 .. 8",
                                           "boundary_frac outside [0, 1] or not finite", "min_games < 1", "t_low or t_high not finite, or t_low > t_high",
                                           "a NULL table", "rows outside 1 .. 64", "a non-finite start_lo, start_hi, limit_lo, limit_hi or step", "step <= 0",
                                           "limit_lo <= 0", "not limit_lo <= start_lo <= start_hi <= limit_hi"};
        if (which >= 0)
            pp_set_errorf("pp_dr_adr_upload: dim %d: %s", which, text[why]);
        else
            pp_set_errorf("pp_dr_adr_upload: %s", text[why]);
        return PPENV_EINVAL;
    }
    pp_dr_adr host = *a;
    host.thr = pp::adr_thr(boundary_frac);
    if (hipMemcpyAsync(adr_dev, &host, sizeof(pp_dr_adr), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {                    // set-up, once: `host` lives on this stack
        (void)hipGetLastError();
        ppenv_set_error("pp_dr_adr_upload: copying the struct to the device failed");
        return PPENV_EHIP;
    }
    return PPENV_OK;
}

extern "C" int pp_dr_adr_fill(const pp_dr_adr* adr_dev, int32_t num_envs, int32_t dims, const pp_dr_adr_state* state, void* stream) {
    if (!adr_dev || !state_ok(state) || num_envs <= 0 || dims < 1 || dims > PPENV_DR_MAX_TABLES) {
        ppenv_set_error("pp_dr_adr_fill: NULL pointer, num_envs <= 0 or dims outside 1 .. 8");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(adr_fill_kernel, dim3(pp_blocks_of(num_envs, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, adr_dev, num_envs, dims, *state);
    return pp_launched("launching adr_fill_kernel failed");
}

extern "C" int pp_dr_adr_step(const pp_dr_adr* adr_dev, int32_t num_envs, const float* rew, const int64_t* reset, const pp_dr_adr_state* state,
                              int32_t* fin_slot_t, int64_t* fin_q_t, void* stream) {
    if (!adr_dev || !rew || !reset || !state_ok(state) || !fin_slot_t || !fin_q_t || num_envs <= 0) {
        ppenv_set_error("pp_dr_adr_step: NULL pointer or num_envs <= 0");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(adr_step_kernel, dim3(pp_blocks_of(num_envs, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, adr_dev, num_envs, rew, reset, *state,
                       fin_slot_t, fin_q_t);
    return pp_launched("launching adr_step_kernel failed");
}

extern "C" int pp_dr_adr_update(const pp_dr_adr* adr_dev, int32_t dims, const int64_t* tot, const pp_dr_adr_state* state, void* stream) {
    if (!adr_dev || !tot || !state_ok(state) || dims < 1 || dims > PPENV_DR_MAX_TABLES) {
        ppenv_set_error("pp_dr_adr_update: NULL pointer or dims outside 1 .. 8");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(adr_update_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, adr_dev, dims, tot, *state);
    return pp_launched("launching adr_update_kernel failed");
}
