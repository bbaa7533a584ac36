// ppenv_play_pair.hip — paired episode statistics on the device (include/ppenv_play_pair.h): the first M episodes of every env of G
// groups in a table, and per cell the fp64 sums of the paired difference against a baseline cell.
//
// Bound by launch latency like ppenv_play.hip: a control step moves 20-30 B per env.
//   play_pair_record_kernel   one lane per env, every step: the per-env step of ppenv_play_pair_device.h.  An env reads and writes its
//                             own words alone.
//   play_pair_reduce_kernel   at polls only: workgroup g is cell g; lane l sums the pairs l, l + 256, ... in order, an xor butterfly
//                             within the wave (strides 32 down to 1), the four waves in order through LDS (ppenv_reduce_device.h),
//                             thread 0 OVERWRITES out[g].  It reads the table and writes out[g] alone: idempotent.
//   play_pair_reset_kernel    one lane per table entry: ret to quiet NaN, everything else to zero.
// No atomics, no hand-off between workgroups; every sum has a fixed order.
//
// This unit's flags (isaacgym_amd/_lib.py): -ffp-contract=off (d * d is rounded before it is added, as in the host build), signed
// zeros kept, and no -ffinite-math-only (the table starts as NaN).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_play_pair_device.h"
#include "ppenv_reduce_device.h"

#include "ppenv_play_host.h"

namespace {

constexpr int kBlock = PPENV_PLAY_BLOCK;
constexpr int kWaves = kBlock / 64;

struct Merge {
    __device__ void operator()(pp_play_pair_totals& into, const pp_play_pair_totals& from) const { pp::play_pair_merge(into, from); }
};

__global__ __launch_bounds__(kBlock) void play_pair_record_kernel(const float* __restrict__ rew, const int64_t* __restrict__ done, int32_t num_envs,
                                                                  int32_t num_agents, int32_t episodes, float* __restrict__ cur_reward,
                                                                  int32_t* __restrict__ cur_steps, int32_t* __restrict__ count, float* __restrict__ ret,
                                                                  int32_t* __restrict__ len) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < num_envs) pp::play_pair_env((int32_t)e, num_agents, episodes, rew, done, cur_reward, cur_steps, count, ret, len);
}

__global__ __launch_bounds__(kBlock) void play_pair_reduce_kernel(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes,
                                                                  const int32_t* __restrict__ baseline, const int32_t* __restrict__ count,
                                                                  const float* __restrict__ ret, const int32_t* __restrict__ len,
                                                                  pp_play_pair_totals* __restrict__ out) {
    __shared__ pp_play_pair_totals wave_part[kWaves];
    const int32_t g = (int32_t)blockIdx.x, b = baseline[g];
    pp_play_pair_totals acc;
    pp::play_pair_clear(acc);
    const bool ok = pp::play_pair_baseline_ok(b, groups);        // uniform in the workgroup
    if (ok) pp::play_pair_lane((int)threadIdx.x, kBlock, g, b, envs_per_group, num_agents, episodes, count, ret, len, acc);
    if (pp::block_reduce(acc, wave_part, Merge())) {
        if (!ok) acc.pairs = -1;
        out[g] = acc;
    }
}

__global__ __launch_bounds__(kBlock) void play_pair_reset_kernel(int64_t n_ret, int64_t n_len, int64_t rows, int64_t num_envs, float* __restrict__ cur_reward,
                                                                 int32_t* __restrict__ cur_steps, int32_t* __restrict__ count, float* __restrict__ ret,
                                                                 int32_t* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;    // num_envs <= rows <= n_ret and n_len <= n_ret: the grid covers them
    if (i < n_ret) ret[i] = pp::play_pair_nan();
    if (i < n_len) len[i] = 0;
    if (i < rows) cur_reward[i] = 0.0f;
    if (i < num_envs) {
        cur_steps[i] = 0;
        count[i] = 0;
    }
}

bool sizes_ok(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes) {
    return pp_play_sizes_ok(envs_per_group, groups, num_agents) && episodes >= 1 &&
           (int64_t)envs_per_group * groups * num_agents <= INT32_MAX / (int64_t)episodes;        // the table's entries
}

const char kSizes[] = "groups outside 1..1024, envs_per_group < 1, num_agents not 1 or 2, episodes < 1, or more than 2^31 - 1 table entries";

}  // namespace

extern "C" size_t pp_play_pair_ret_bytes(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes) {
    return sizes_ok(envs_per_group, groups, num_agents, episodes) ? (size_t)envs_per_group * groups * episodes * num_agents * sizeof(float) : 0;
}

extern "C" size_t pp_play_pair_len_bytes(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes) {
    return sizes_ok(envs_per_group, groups, num_agents, episodes) ? (size_t)envs_per_group * groups * episodes * sizeof(int32_t) : 0;
}

extern "C" int pp_play_pair_reset(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes, float* cur_reward, int32_t* cur_steps,
                                  int32_t* count, float* ret, int32_t* len, void* stream) {
    if (!sizes_ok(envs_per_group, groups, num_agents, episodes) || !cur_reward || !cur_steps || !count || !ret || !len) {
        pp_set_errorf("pp_play_pair_reset: NULL pointer, %s", kSizes);
        return PPENV_EINVAL;
    }
    const int64_t num_envs = (int64_t)envs_per_group * groups, rows = num_envs * num_agents, n_len = num_envs * episodes, n_ret = n_len * num_agents;
    hipLaunchKernelGGL(play_pair_reset_kernel, dim3(pp_blocks_of(n_ret, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n_ret, n_len, rows, num_envs, cur_reward,
                       cur_steps, count, ret, len);
    return pp_launched("launching play_pair_reset_kernel failed");
}

extern "C" int pp_play_pair_record(const float* rew, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes,
                                   float* cur_reward, int32_t* cur_steps, int32_t* count, float* ret, int32_t* len, void* stream) {
    if (!sizes_ok(envs_per_group, groups, num_agents, episodes) || !rew || !done || !cur_reward || !cur_steps || !count || !ret || !len) {
        pp_set_errorf("pp_play_pair_record: NULL pointer, %s", kSizes);
        return PPENV_EINVAL;
    }
    const int32_t num_envs = envs_per_group * groups;
    hipLaunchKernelGGL(play_pair_record_kernel, dim3(pp_blocks_of(num_envs, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, rew, done, num_envs, num_agents, episodes,
                       cur_reward, cur_steps, count, ret, len);
    return pp_launched("launching play_pair_record_kernel failed");
}

extern "C" int pp_play_pair_reduce(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes, const int32_t* baseline,
                                   const int32_t* count, const float* ret, const int32_t* len, pp_play_pair_totals* out, void* stream) {
    if (!sizes_ok(envs_per_group, groups, num_agents, episodes) || !baseline || !count || !ret || !len || !out) {
        pp_set_errorf("pp_play_pair_reduce: NULL pointer, %s", kSizes);
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(play_pair_reduce_kernel, dim3((uint32_t)groups), dim3(kBlock), 0, (hipStream_t)stream, envs_per_group, groups, num_agents, episodes,
                       baseline, count, ret, len, out);
    return pp_launched("launching play_pair_reduce_kernel failed");
}
