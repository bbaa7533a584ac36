// ppenv_play.hip — episode accounting for playing a checkpoint, on the device: G populations of S envs, each with its own totals and
// its own freeze (include/ppenv_play_group.h); the single accounting (include/ppenv_play.h) is G = 1, S = num_envs of the same kernels.
//
// Bound by launch latency, not bytes: a control step moves 12-20 B per row.  Two launches per step whatever G is, the shape of
// ppo_loss_grad_kernel / ppo_loss_reduce_kernel:
//   play_rows_kernel     workgroup (x, y) of a P x G grid is chunk x of group y (P = chunks of 256 envs in S, counted from the group's first
//                        env, ragged last chunk per group guarded); a lane owns one env: the per-env step of ppenv_play_device.h, then the workgroup's
//                        finished games summed in a fixed order (ppenv_reduce_device.h: xor butterfly within a wave, strides 32 down to 1,
//                        the four waves in order through LDS) into ONE ppenv_play_partial.  Reads totals[g].games for the freeze; writes no word of the totals.
//   play_totals_kernel   one wave per group: lane l sums the group's partials l, l + 64, ... in order, a butterfly, lane 0 adds the result
//                        to totals[g].
// The totals are written by the second launch only, and wave g of it reads and writes totals[g] alone: nothing a workgroup reads is
// written by another one in the same launch, without atomics, tickets or device-scope fences (such a hand-off costs more than
// the launch boundary).  An env's lane, wave and chunk depend on its index within its group alone, so a group's sums are bit for bit
// those of a run of its S envs by themselves.
//
// -ffinite-math-only is NOT in this unit's flags (isaacgym_amd/_lib.py): the minima / maxima start at +-inf.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_play_device.h"
#include "ppenv_reduce_device.h"
#include "../../include/ppenv_play_group.h"

#include "ppenv_play_host.h"

namespace {

constexpr int kBlock = PPENV_PLAY_BLOCK;
constexpr int kWaves = kBlock / 64;

struct Merge {
    __device__ void operator()(ppenv_play_partial& into, const ppenv_play_partial& from) const { pp::play_merge(into, from); }
};

// Workgroup (x, y) is chunk x of group y: a workgroup belongs to one group, so the freeze test is uniform in it.
__global__ __launch_bounds__(kBlock) void play_rows_kernel(const float* __restrict__ rew, const int64_t* __restrict__ done, int32_t envs_per_group,
                                                           int32_t parts, int32_t num_agents, int64_t games_num, float* __restrict__ cur_reward,
                                                           int32_t* __restrict__ cur_steps, const ppenv_play_totals* __restrict__ totals,
                                                           ppenv_play_partial* __restrict__ partial) {
    __shared__ ppenv_play_partial wave_part[kWaves];
    const int32_t g = (int32_t)blockIdx.y, chunk = (int32_t)blockIdx.x;
    if (pp::play_frozen(totals[g].games, games_num)) return;     // uniform: the whole workgroup leaves (its partial is not read either)
    const int32_t local = chunk * kBlock + (int32_t)threadIdx.x;     // the env's index within its group
    ppenv_play_partial acc;
    pp::play_clear(acc);
    if (local < envs_per_group) pp::play_env(g * envs_per_group + local, num_agents, rew, done, cur_reward, cur_steps, acc);
    if (pp::block_reduce(acc, wave_part, Merge())) partial[g * parts + chunk] = acc;
}

__global__ __launch_bounds__(64) void play_totals_kernel(const ppenv_play_partial* __restrict__ partial, int32_t parts, int64_t games_num,
                                                         ppenv_play_totals* __restrict__ totals) {
    const int32_t g = (int32_t)blockIdx.x;
    if (pp::play_frozen(totals[g].games, games_num)) return;     // the word the group's chunks tested: nothing wrote it in between
    const ppenv_play_partial* mine = partial + (size_t)g * parts;
    ppenv_play_partial acc;
    pp::play_clear(acc);
    for (int32_t b = (int32_t)threadIdx.x; b < parts; b += 64) pp::play_merge(acc, mine[b]);
    pp::wave_butterfly(acc, Merge());
    if (threadIdx.x == 0) {
        ppenv_play_totals t = totals[g];
        pp::play_totals_add(t, acc);
        totals[g] = t;
    }
}

__global__ __launch_bounds__(kBlock) void play_reset_kernel(int32_t num_envs, int32_t rows, int32_t groups, float* __restrict__ cur_reward,
                                                            int32_t* __restrict__ cur_steps, ppenv_play_totals* __restrict__ totals) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i < rows) cur_reward[i] = 0.0f;
    if (i < num_envs) cur_steps[i] = 0;
    if (i < groups) {                                            // groups <= num_envs <= rows: the grid covers them
        ppenv_play_totals t;
        pp::play_totals_clear(t);
        totals[i] = t;
    }
}

// The launches, after the entry's own validation.
int launch_reset(int32_t envs_per_group, int32_t groups, int32_t num_agents, float* cur_reward, int32_t* cur_steps, ppenv_play_totals* totals, void* stream) {
    const int32_t num_envs = envs_per_group * groups, rows = num_envs * num_agents;
    hipLaunchKernelGGL(play_reset_kernel, dim3(pp_blocks_of(rows, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, num_envs, rows, groups, cur_reward, cur_steps, totals);
    return pp_launched("launching play_reset_kernel failed");
}

int launch_accumulate(const float* rew, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents, int64_t games_num, float* cur_reward,
                      int32_t* cur_steps, ppenv_play_totals* totals, ppenv_play_partial* partial, void* stream) {
    const int32_t parts = pp_blocks_of(envs_per_group, kBlock);  // per group; groups * parts <= 2^31 / 256 workgroups
    hipLaunchKernelGGL(play_rows_kernel, dim3((uint32_t)parts, (uint32_t)groups), dim3(kBlock), 0, (hipStream_t)stream, rew, done, envs_per_group, parts,
                       num_agents, games_num, cur_reward, cur_steps, totals, partial);
    if (int rc = pp_launched("launching play_rows_kernel failed")) return rc;
    hipLaunchKernelGGL(play_totals_kernel, dim3(groups), dim3(64), 0, (hipStream_t)stream, partial, parts, games_num, totals);
    return pp_launched("launching play_totals_kernel failed");
}

}  // namespace

// ---- the plain entries (include/ppenv_play.h): one population, the G = 1 case ------------------------------------------------------------
extern "C" size_t ppenv_play_partial_bytes(int32_t num_envs) {
    return num_envs > 0 ? (size_t)pp_blocks_of(num_envs, kBlock) * sizeof(ppenv_play_partial) : 0;
}

extern "C" int ppenv_play_reset(int32_t num_envs, int32_t num_agents, float* cur_reward, int32_t* cur_steps, ppenv_play_totals* totals, void* stream) {
    if (!pp_play_sizes_ok(num_envs, 1, num_agents) || !cur_reward || !cur_steps || !totals) {
        ppenv_set_error("ppenv_play_reset: NULL pointer, num_envs <= 0, num_agents not 1 or 2, or more than 2^31 - 1 rows");
        return PPENV_EINVAL;
    }
    return launch_reset(num_envs, 1, num_agents, cur_reward, cur_steps, totals, stream);
}

extern "C" int ppenv_play_accumulate(const float* rew, const int64_t* done, int32_t num_envs, int32_t num_agents, int64_t games_num, float* cur_reward,
                                     int32_t* cur_steps, ppenv_play_totals* totals, ppenv_play_partial* partial, void* stream) {
    if (!pp_play_sizes_ok(num_envs, 1, num_agents) || !rew || !done || !cur_reward || !cur_steps || !totals || !partial || games_num < 1) {
        ppenv_set_error("ppenv_play_accumulate: NULL pointer, num_envs <= 0, num_agents not 1 or 2, more than 2^31 - 1 rows, or games_num < 1");
        return PPENV_EINVAL;
    }
    return launch_accumulate(rew, done, num_envs, 1, num_agents, games_num, cur_reward, cur_steps, totals, partial, stream);
}

// ---- the grouped entries (include/ppenv_play_group.h): G populations of S envs, each with its own totals and its own freeze -------------
extern "C" size_t pp_play_group_partial_bytes(int32_t envs_per_group, int32_t groups) {
    return pp_play_sizes_ok(envs_per_group, groups, 1) ? (size_t)groups * (size_t)pp_blocks_of(envs_per_group, kBlock) * sizeof(ppenv_play_partial) : 0;
}

extern "C" int pp_play_group_reset(int32_t envs_per_group, int32_t groups, int32_t num_agents, float* cur_reward, int32_t* cur_steps,
                                   ppenv_play_totals* totals, void* stream) {
    if (!pp_play_sizes_ok(envs_per_group, groups, num_agents) || !cur_reward || !cur_steps || !totals) {
        ppenv_set_error("pp_play_group_reset: NULL pointer, groups outside 1..1024, envs_per_group <= 0, num_agents not 1 or 2, or more than 2^31 - 1 rows");
        return PPENV_EINVAL;
    }
    return launch_reset(envs_per_group, groups, num_agents, cur_reward, cur_steps, totals, stream);
}

extern "C" int pp_play_group_accumulate(const float* rew, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents, int64_t games_num,
                                        float* cur_reward, int32_t* cur_steps, ppenv_play_totals* totals, ppenv_play_partial* partial, void* stream) {
    if (!pp_play_sizes_ok(envs_per_group, groups, num_agents) || !rew || !done || !cur_reward || !cur_steps || !totals || !partial || games_num < 1) {
        ppenv_set_error("pp_play_group_accumulate: NULL pointer, groups outside 1..1024, envs_per_group <= 0, num_agents not 1 or 2, more than 2^31 - 1 rows, "
                        "or games_num < 1");
        return PPENV_EINVAL;
    }
    return launch_accumulate(rew, done, envs_per_group, groups, num_agents, games_num, cur_reward, cur_steps, totals, partial, stream);
}
