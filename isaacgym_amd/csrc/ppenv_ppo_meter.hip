// ppenv_ppo_meter.hip — the trainer's score meter on the device (include/ppenv_ppo_meter.h): rl_games' AverageMeter(games_to_track) of the
// finished games' returns and lengths, once per epoch over the collector's horizon.
//
// Bound by launch latency, not bytes: a horizon of 32 x 4096 moves 1.5 MB.  Two launches, the shape of play_rows_kernel /
// play_totals_kernel:
//   meter_rows_kernel    lane e owns env e (256 envs per workgroup, ragged tail guarded) and walks t = 0 .. h-1 with its running return and
//                        length in registers, kChunk steps at a time: the chunk's rewards and done words are loaded first (independent
//                        loads, one wait), then per step the wave's finished games are summed by an xor butterfly (ppenv_reduce_device.h,
//                        strides 32 down to 1; skipped, wave-uniformly, when no lane finished) and left in LDS; after the chunk one lane
//                        per step adds the four waves in order and writes the workgroup's ppenv_ppo_meter_partial for that step.
//   meter_update_kernel  one wave, for t in order: lane l sums partials l, l + 64, ... in order, a butterfly, AverageMeter.update.
// The meter is written by the second launch only, which has one workgroup; cur_reward / cur_len and the partials are written by the
// lane / workgroup that owns them: nothing a workgroup reads is written by another one in the same launch, without atomics, tickets
// or device-scope fences.
//
// This unit's flags (isaacgym_amd/_lib.py SOURCE_FLAGS): -ffp-contract=off, signed zeros and no -ffinite-math-only — the update's
// operations round one by one, as the host build of ppenv_ppo_meter_device.h does.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_ppo_meter_device.h"
#include "ppenv_reduce_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = PPENV_PPO_METER_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 16;                         // steps whose rewards and done words a lane holds at once

struct Merge {
    __device__ void operator()(ppenv_ppo_meter_partial& into, const ppenv_ppo_meter_partial& from) const { pp::meter_merge(into, from); }
};

__global__ __launch_bounds__(kBlock) void meter_rows_kernel(const float* __restrict__ rew, int64_t ld_rew, const int64_t* __restrict__ done,
                                                            int64_t ld_done, int32_t h, int32_t num_envs, int32_t num_agents,
                                                            float* __restrict__ cur_reward, int32_t* __restrict__ cur_len,
                                                            ppenv_ppo_meter_partial* __restrict__ partial, int32_t parts) {
    __shared__ ppenv_ppo_meter_partial wave_part[kChunk][kWaves];
    const int tid = threadIdx.x;
    const int32_t e = (int32_t)(blockIdx.x * kBlock + tid);
    const bool live = e < num_envs;
    const size_t col = (size_t)num_agents * (size_t)(live ? e : 0);      // agent 0's row of the env
    float cr = live ? cur_reward[e] : 0.0f;
    int32_t cl = live ? cur_len[e] : 0;
    for (int32_t t0 = 0; t0 < h; t0 += kChunk) {
        const int32_t nt = h - t0 < kChunk ? h - t0 : kChunk;
        float r[kChunk];
        int64_t d[kChunk];
        #pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            const bool in = live && j < nt;
            r[j] = in ? rew[(size_t)(t0 + j) * (size_t)ld_rew + col] : 0.0f;
            d[j] = in ? done[(size_t)(t0 + j) * (size_t)ld_done + col] : 0;
        }
        #pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            if (j < nt) {                                                // uniform
                ppenv_ppo_meter_partial fin;
                pp::meter_clear(fin);
                if (live) pp::meter_env_step(r[j], d[j], cr, cl, fin);
                // wave-uniform; without it lane 0 holds zeros: no lane finished
                if (__ballot(fin.count != 0) != 0ull) pp::wave_butterfly(fin, Merge());
                pp::wave_store(wave_part[j], fin);
            }
        }
        __syncthreads();
        if (tid < nt) partial[(size_t)(t0 + tid) * (size_t)parts + blockIdx.x] = pp::waves_in_order(wave_part[tid], Merge());
        __syncthreads();                                                 // the next chunk rewrites wave_part
    }
    if (live) {
        cur_reward[e] = cr;
        cur_len[e] = cl;
    }
}

__global__ __launch_bounds__(64) void meter_update_kernel(const ppenv_ppo_meter_partial* __restrict__ partial, int32_t parts, int32_t h,
                                                          int64_t games_to_track, ppenv_ppo_meter* __restrict__ meter) {
    ppenv_ppo_meter m = *meter;                                          // every lane carries the same meter
    for (int32_t t = 0; t < h; ++t) {
        ppenv_ppo_meter_partial acc;
        pp::meter_clear(acc);
        for (int32_t b = (int32_t)threadIdx.x; b < parts; b += 64) pp::meter_merge(acc, partial[(size_t)t * (size_t)parts + b]);
        if (__ballot(acc.count != 0) == 0ull) continue;                  // wave-uniform: nobody finished at t
        pp::wave_butterfly(acc, Merge());
        pp::meter_apply(m, acc, games_to_track);
    }
    if (threadIdx.x == 0) *meter = m;
}

}  // namespace

extern "C" size_t ppo_meter_partial_bytes(int32_t h, int32_t num_envs) {
    return h > 0 && num_envs > 0 ? (size_t)h * (size_t)pp_blocks_of(num_envs, kBlock) * sizeof(ppenv_ppo_meter_partial) : 0;
}

extern "C" int ppo_meter_update(const float* rew, int64_t ld_rew, const int64_t* done, int64_t ld_done, int32_t h, int32_t num_envs, int32_t num_agents,
                                int64_t games_to_track, float* cur_reward, int32_t* cur_len, ppenv_ppo_meter* meter, ppenv_ppo_meter_partial* partial,
                                void* stream) {
    const int64_t rows = (int64_t)num_envs * num_agents;
    if (!rew || !done || !cur_reward || !cur_len || !meter || !partial || h < 1 || num_envs < 1 || num_agents < 1 || num_agents > 2 ||
        rows > INT32_MAX || ld_rew < rows || ld_done < rows || games_to_track < 1) {
        ppenv_set_error("ppo_meter_update: NULL pointer, h < 1, num_envs < 1, num_agents not 1 or 2, more than 2^31 - 1 rows, a row stride below "
                        "num_agents x num_envs, or games_to_track < 1");
        return PPENV_EINVAL;
    }
    const int32_t parts = pp_blocks_of(num_envs, kBlock);
    hipLaunchKernelGGL(meter_rows_kernel, dim3(parts), dim3(kBlock), 0, (hipStream_t)stream, rew, ld_rew, done, ld_done, h, num_envs, num_agents,
                       cur_reward, cur_len, partial, parts);
    if (int rc = pp_launched("launching meter_rows_kernel failed")) return rc;
    hipLaunchKernelGGL(meter_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const ppenv_ppo_meter_partial*)partial, parts, h, games_to_track,
                       meter);
    return pp_launched("launching meter_update_kernel failed");
}
