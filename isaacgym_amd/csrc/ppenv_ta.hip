// ppenv_ta.hip — 27-DoF variant, tensor-API mode: post_physics_step of
// tasks/humanoid_pingpong_3_actor_all_dof.py ("TA") TA:1145-1192 on caller-supplied simulator tensors.
// One lane per env; every op is fp32 in the reference's operation order (IEEE division / sqrt / expf).
// The per-env arithmetic is ppenv_ta_task.h (shared with the fused step of ppenv_ta_sim.hip).
#undef PP_STAMP   // the phase stamps of diagnostic builds belong to ppenv.hip's kernels
#include <hip/hip_runtime.h>

#include <cstdio>

#include "ppenv_ta_task.h"
#include "ppenv_ta_outcome_device.h"

using namespace pp;

namespace {

constexpr int kTaBlock = 16;   // one lane per env with strided AoS rows: small workgroups spread the envs over all CUs (4096 envs -> 256 workgroups)
__global__ __launch_bounds__(kTaBlock) void ta_post_physics_kernel(const ppenv_ta_params p, const float* __restrict__ rb_states,
                                                                    const float* __restrict__ initial_rb_states, float* root_states,
                                                                    float* dof_states, const float* __restrict__ dof_force,
                                                                    const float* __restrict__ pre_ball_vx,
                                                                    const float* __restrict__ reset_override, uint32_t* flags,
                                                                    uint32_t* episode, long long* progress, float* obs, float* rew,
                                                                    long long* reset_out, uint32_t* any_reset) {
    const int n = p.num_envs;
    const int i = blockIdx.x * kTaBlock + threadIdx.x;
    if (i >= n) return;
    tatask::ta_task_env<1>(p, i, rb_states + (size_t)i * PPENV_NUM_BODIES * 13, initial_rb_states + (size_t)(p.initial_rb_shared ? 0 : i) * PPENV_NUM_BODIES * 13,
                        root_states + (size_t)i * PPENV_NUM_ACTORS * 13, dof_states + (size_t)i * tatask::TA_ND * 2, dof_force + (size_t)i * tatask::TA_ND,
                        pre_ball_vx[i], reset_override ? reset_override + (size_t)i * 5 : nullptr, &flags[i], &episode[i], &progress[i],
                        obs + (size_t)i * PPENV_TA_NUM_OBS, &rew[i], &reset_out[i], any_reset, 0, true);
}

// TA:1162-1166: whenever ANY env resets, the diagnostic count flags of ALL envs are cleared
// One workgroup: every thread reads the word before the barrier, then it is zeroed for the next step — the step needs no memset
// launch (5.5 us of a 133 us step) as long as the word starts at zero.
// With `outcome` (include/ppenv_ta_outcome.h; NULL: off) the five count bits are summed over all n words before they go: every thread its
// words, a butterfly within the wave, the 16 waves in order through LDS, and thread 0 alone updates the struct (integers: any order
// gives the same bits).  The branch is uniform, and with outcome NULL the kernel does what it did without the feature.
__global__ __launch_bounds__(1024) void ta_clear_counts_kernel(int n, uint32_t* flags, uint32_t* any_reset, pp_ta_outcome* outcome) {
    __shared__ uint32_t wave_sum[16][PP_TA_OUTCOME_COUNTS];
    const bool any = *any_reset != 0u;
    __syncthreads();
    if (threadIdx.x == 0) *any_reset = 0u;
    if (!any) return;
    if (!outcome) {
        for (int i = threadIdx.x; i < n; i += 1024) flags[i] &= ~PPENV_TA_COUNT_MASK;
        return;
    }
    uint32_t c[PP_TA_OUTCOME_COUNTS] = {0u, 0u, 0u, 0u, 0u};
    for (int i = threadIdx.x; i < n; i += 1024) {
        const uint32_t f = flags[i];
        ta_outcome_word(f, c);
        flags[i] = f & ~PPENV_TA_COUNT_MASK;
    }
#pragma unroll
    for (int k = 0; k < PP_TA_OUTCOME_COUNTS; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c[k] += __shfl_xor(c[k], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < PP_TA_OUTCOME_COUNTS; ++k) wave_sum[wave][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t[PP_TA_OUTCOME_COUNTS] = {0u, 0u, 0u, 0u, 0u};
        for (int w = 0; w < 16; ++w) {
#pragma unroll
            for (int k = 0; k < PP_TA_OUTCOME_COUNTS; ++k) t[k] += wave_sum[w][k];
        }
        pp_ta_outcome o = *outcome;
        ta_outcome_window(o, (uint64_t)n, t);
        *outcome = o;
    }
}

// include/ppenv_ta_outcome.h: *latched = *live while the play totals are not frozen.  One wave; lane w copies 8-byte word w.
__global__ __launch_bounds__(64) void ta_outcome_latch_kernel(const pp_ta_outcome* __restrict__ live, const ppenv_play_totals* __restrict__ totals,
                                                              int64_t games_num, pp_ta_outcome* __restrict__ latched) {
    if (!ta_outcome_latches(totals->games, games_num)) return;       // uniform
    constexpr int kWords = (int)(sizeof(pp_ta_outcome) / sizeof(uint64_t));
    static_assert(kWords <= 64, "one lane per word");
    if ((int)threadIdx.x < kWords) reinterpret_cast<uint64_t*>(latched)[threadIdx.x] = reinterpret_cast<const uint64_t*>(live)[threadIdx.x];
}

// ---- 4-actor variant: compute_humanoid1_pingpong_reward (== TT's, T4:1113-1278) and its mirror
// compute_humanoid2_pingpong_reward T4:1280-1439, both sides in one launch
__global__ __launch_bounds__(kTaBlock) void t4_rewards_kernel(const ppenv_t4_params p, const float* __restrict__ rb_states,
                                                               const float* __restrict__ root_states, const float* __restrict__ dof_states,
                                                               const float* __restrict__ dof_force, const float* __restrict__ pre_ball_vx,
                                                               const long long* __restrict__ progress, const uint32_t* __restrict__ flags1_in,
                                                               const uint32_t* __restrict__ flags2_in, uint32_t* flags1, uint32_t* flags2,
                                                               float* rew1, float* rew2, long long* reset1, long long* reset2) {
    const int i = blockIdx.x * kTaBlock + threadIdx.x;
    if (i >= p.num_envs) return;
    const float* rb = rb_states + (size_t)i * PPENV_T4_NUM_BODIES * 13;
    const float* root = root_states + (size_t)i * PPENV_T4_NUM_ACTORS * 13;
    const float* ball = root + 3 * 13;
    float power = 0.f;
#pragma unroll
    for (int d = 0; d < PPENV_T4_NUM_DOF; d++)   // the class hands the whole 14-dof tensors to the reward (T4:746-747)
        power += fabsf(dof_force[(size_t)i * PPENV_T4_NUM_DOF + d] * dof_states[((size_t)i * PPENV_T4_NUM_DOF + d) * 2 + 1]);
    const V3 bp = mk(ball[0], ball[1], ball[2]);
    // side 1 = TT's function verbatim (T4:1113-1278 == TT:1105-1270): the shared compute_reward with TT semantics
    RewardConsts c;
    c.variant = PPENV_VARIANT_TT;
    c.max_episode_length = p.max_episode_length;
    c.alpha = p.alpha_velocity_reward; c.power_coefficient = p.power_coefficient; c.penalty = p.penalty;
    c.hit_table_reward = p.hit_table_reward; c.not_hit_table_penalty = p.not_hit_table_penalty;
    RewardIn in;
    in.humanoid_x = root[0];
    in.paddle = mk(rb[39 * 13], rb[39 * 13 + 1], rb[39 * 13 + 2]);
    in.pre_vx = pre_ball_vx[i];
    in.bp = bp;
    in.vx = ball[7];
    in.power = power;
    in.progress = progress[i];
    uint32_t f1 = flags1_in[i], f2 = flags2_in[i];
    long long r1, r2;
    rew1[i] = compute_reward(c, in, f1, r1);
    RewardIn in2 = in;
    in2.humanoid_x = root[13];
    in2.paddle = mk(rb[79 * 13], rb[79 * 13 + 1], rb[79 * 13 + 2]);
    rew2[i] = compute_reward_side2(c, in2, f2, r2);
    flags1[i] = f1; flags2[i] = f2; reset1[i] = r1; reset2[i] = r2;
}

}  // namespace

#include "ppenv_host.h"

namespace {
// The stateless entries have no handle to remember a device: they launch on the device that owns their output tensor, whatever the
// caller's current device is (a rank that never called hipSetDevice would otherwise launch on device 0 with another device's pointers).
int use_device_of(const void* dev_ptr) {
    hipPointerAttribute_t at;
    int cur = -1;
    if (hipPointerGetAttributes(&at, dev_ptr) != hipSuccess || hipGetDevice(&cur) != hipSuccess) {
        (void)hipGetLastError();
        ppenv_set_error("could not determine the device of the output tensor (is it a device pointer?)");
        return PPENV_EINVAL;
    }
    if (at.device != cur && hipSetDevice(at.device) != hipSuccess) { ppenv_set_error("hipSetDevice to the output tensor's device failed"); return PPENV_EHIP; }
    return PPENV_OK;
}
}  // namespace

// TA:1162-1166 as a launch of its own (also used by the fused step of ppenv_ta_sim.hip); not part of the public ABI
int ppenv_ta_clear_counts(int n, uint32_t* flags_dev, uint32_t* any_reset_dev, pp_ta_outcome* outcome_dev, void* stream) {
    hipLaunchKernelGGL(ta_clear_counts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, flags_dev, any_reset_dev, outcome_dev);
    return pp_launched("launching ta_clear_counts_kernel failed");
}

extern "C" int ppenv_t4_rewards(const ppenv_t4_params* params, const float* rb_states_dev, const float* root_states_dev,
                                const float* dof_states_dev, const float* dof_force_dev, const float* pre_ball_vx_dev,
                                const int64_t* progress_dev, const uint32_t* flags1_in_dev, const uint32_t* flags2_in_dev,
                                uint32_t* flags1_dev, uint32_t* flags2_dev, float* rew1_dev, float* rew2_dev, int64_t* reset1_dev,
                                int64_t* reset2_dev, void* stream) {
    if (!params || params->num_envs <= 0 || !rb_states_dev || !root_states_dev || !dof_states_dev || !dof_force_dev || !pre_ball_vx_dev ||
        !progress_dev || !flags1_in_dev || !flags2_in_dev || !flags1_dev || !flags2_dev || !rew1_dev || !rew2_dev || !reset1_dev || !reset2_dev) {
        ppenv_set_error("ppenv_t4_rewards: NULL argument or num_envs <= 0");
        return PPENV_EINVAL;
    }
    const int n = params->num_envs;
    if (int rc = use_device_of(rew1_dev)) return rc;
    hipLaunchKernelGGL(t4_rewards_kernel, dim3((n + kTaBlock - 1) / kTaBlock), dim3(kTaBlock), 0, (hipStream_t)stream, *params, rb_states_dev,
                       root_states_dev, dof_states_dev, dof_force_dev, pre_ball_vx_dev, (const long long*)progress_dev, flags1_in_dev, flags2_in_dev, flags1_dev, flags2_dev,
                       rew1_dev, rew2_dev, (long long*)reset1_dev, (long long*)reset2_dev);
    return pp_launched("launching t4_rewards_kernel failed");
}

namespace {
int ta_post_physics(const char* who, const ppenv_ta_params* params, const float* rb_states_dev, const float* initial_rb_states_dev, float* root_states_dev,
                    float* dof_states_dev, const float* dof_force_dev, const float* pre_ball_vx_dev, const float* reset_override_dev, uint32_t* flags_dev,
                    uint32_t* episode_dev, int64_t* progress_dev, float* obs_dev, float* rew_dev, int64_t* reset_dev, uint32_t* scratch_any_reset_dev,
                    pp_ta_outcome* outcome_dev, void* stream) {
    if (!params || params->num_envs <= 0 || !rb_states_dev || !initial_rb_states_dev || !root_states_dev || !dof_states_dev ||
        !dof_force_dev || !pre_ball_vx_dev || !flags_dev || !episode_dev || !progress_dev || !obs_dev || !rew_dev || !reset_dev ||
        !scratch_any_reset_dev) {
        pp_set_errorf("%s: NULL argument or num_envs <= 0", who);
        return PPENV_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(outcome_dev) & 7) { pp_set_errorf("%s: the outcome struct must be 8-byte aligned", who); return PPENV_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int n = params->num_envs;
    if (int rc = use_device_of(obs_dev)) return rc;
    hipLaunchKernelGGL(ta_post_physics_kernel, dim3((n + kTaBlock - 1) / kTaBlock), dim3(kTaBlock), 0, s, *params, rb_states_dev,
                       initial_rb_states_dev, root_states_dev, dof_states_dev, dof_force_dev, pre_ball_vx_dev, reset_override_dev, flags_dev,
                       episode_dev, (long long*)progress_dev, obs_dev, rew_dev, (long long*)reset_dev, scratch_any_reset_dev);
    hipLaunchKernelGGL(ta_clear_counts_kernel, dim3(1), dim3(1024), 0, s, n, flags_dev, scratch_any_reset_dev, outcome_dev);
    return pp_launched("launching the TA post-physics kernels failed");
}
}  // namespace

extern "C" int ppenv_ta_post_physics_step(const ppenv_ta_params* params, const float* rb_states_dev, const float* initial_rb_states_dev,
                                          float* root_states_dev, float* dof_states_dev, const float* dof_force_dev,
                                          const float* pre_ball_vx_dev, const float* reset_override_dev, uint32_t* flags_dev,
                                          uint32_t* episode_dev, int64_t* progress_dev, float* obs_dev, float* rew_dev, int64_t* reset_dev,
                                          uint32_t* scratch_any_reset_dev, void* stream) {
    return ta_post_physics("ppenv_ta_post_physics_step", params, rb_states_dev, initial_rb_states_dev, root_states_dev, dof_states_dev, dof_force_dev,
                           pre_ball_vx_dev, reset_override_dev, flags_dev, episode_dev, progress_dev, obs_dev, rew_dev, reset_dev, scratch_any_reset_dev,
                           nullptr, stream);
}

extern "C" int pp_ta_post_physics_step_outcome(const ppenv_ta_params* params, const float* rb_states_dev, const float* initial_rb_states_dev,
                                               float* root_states_dev, float* dof_states_dev, const float* dof_force_dev,
                                               const float* pre_ball_vx_dev, const float* reset_override_dev, uint32_t* flags_dev,
                                               uint32_t* episode_dev, int64_t* progress_dev, float* obs_dev, float* rew_dev, int64_t* reset_dev,
                                               uint32_t* scratch_any_reset_dev, pp_ta_outcome* outcome_dev, void* stream) {
    return ta_post_physics("pp_ta_post_physics_step_outcome", params, rb_states_dev, initial_rb_states_dev, root_states_dev, dof_states_dev, dof_force_dev,
                           pre_ball_vx_dev, reset_override_dev, flags_dev, episode_dev, progress_dev, obs_dev, rew_dev, reset_dev, scratch_any_reset_dev,
                           outcome_dev, stream);
}

extern "C" int pp_ta_outcome_latch(const pp_ta_outcome* live, const ppenv_play_totals* totals, int64_t games_num, pp_ta_outcome* latched, void* stream) {
    if (!live || !totals || !latched || games_num < 1 || ((reinterpret_cast<uintptr_t>(live) | reinterpret_cast<uintptr_t>(latched)) & 7)) {
        ppenv_set_error("pp_ta_outcome_latch: NULL pointer, a struct that is not 8-byte aligned, or games_num < 1");
        return PPENV_EINVAL;
    }
    if (int rc = use_device_of(latched)) return rc;
    hipLaunchKernelGGL(ta_outcome_latch_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, live, totals, games_num, latched);
    return pp_launched("launching ta_outcome_latch_kernel failed");
}
