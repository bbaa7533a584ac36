/*
 * ppenv_ppo_meter.h — C ABI of the trainer's score meter: rl_games' running mean of the last `games_to_track` finished games
 * (a2c_common's game_rewards / game_lengths, algos_torch.torch_ext.AverageMeter — restated from its published code, rl_games is absent
 * offline: parity unpinned), kept on the device.  cfg/train/HumanoidPingpongTiltG1PPO.yaml:63-65 (score_to_win, save_best_after) are
 * judged by it.
 *
 * rl_games does this inside play_steps, per step, with a `done.nonzero()` on the host.  Here it runs ONCE PER EPOCH over the horizon the
 * collector already holds: rew [h, rows] fp32 (unscaled) and done [h, rows] int64, rows = num_agents * num_envs, row
 * num_agents * e being agent 0 of env e (rl_games' all_done_indices[::num_agents]; only that row is read).  Per env, in step order:
 *
 *     cur_reward[e] = fl32(cur_reward[e] + rew[t, A e]);  cur_len[e] += 1
 *     the env finishes at t when done[t, A e] != 0 (all 64 bits)
 *
 * and per step t in order, with c_t the envs that finished at t, S_t the fp64 sum of their cur_reward and L_t the integer sum of their
 * cur_len: if c_t > 0, AverageMeter.update for both means (W = games_to_track), everything in fp64, every operation rounded on its own:
 *
 *     new_mean = S_t / c_t                       (L_t / c_t for the length)
 *     size     = min(c_t, W)
 *     old      = min(W - size, current_size)
 *     mean     = (mean * old + new_mean * size) / (old + size)
 *     current_size = old + size;  games_total += c_t;  updates += 1
 *
 * then the finished envs' running values restart at zero.  rl_games keeps the meter in fp32 torch with an unspecified summation order;
 * fp64 with a fixed order is this build's stated deviation.
 *
 * Two launches, the shape of ppenv_play_accumulate.  meter_rows_kernel: lane = env, PPENV_PPO_METER_BLOCK envs per workgroup; each lane
 * walks t = 0 .. h-1 with its running values in registers and the workgroup writes one ppenv_ppo_meter_partial per step (xor butterfly
 * within a wave, the four waves in order through LDS).  meter_update_kernel: one wave, for t in order: lane l sums partials l, l + 64, ...
 * in order, a butterfly, lane 0 applies the update.  No word a workgroup reads is written by another one in the same launch; no atomics,
 * tickets or fences; every sum has a fixed order: results are bitwise reproducible run to run.  The launches read no host-side counter:
 * captured in a graph they replay like eager ones.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the message
 * in ppenv_last_error().  The entry points are named ppo_meter_*: the set of ppenv_* entries is pinned by tests/test_abi_errors_host.py.
 */
#ifndef PPENV_PPO_METER_H
#define PPENV_PPO_METER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPENV_PPO_METER_BLOCK 256                     /* envs per workgroup = envs per partial */

/* The games a workgroup's envs finished at one step. */
typedef struct ppenv_ppo_meter_partial {
    double sum;                                       /* of their returns */
    int64_t len;                                      /* of their lengths in steps */
    int32_t count;
    int32_t reserved;
} ppenv_ppo_meter_partial;

/* The meter: all zero at the start. */
typedef struct ppenv_ppo_meter {
    double mean_reward;                               /* running mean of the last current_size games' returns (agent 0's, unscaled) */
    double mean_length;                               /* ... of their lengths in steps */
    int64_t current_size;                             /* games the means stand for: at most games_to_track */
    int64_t games_total;                              /* all games ever finished */
    int64_t updates;                                  /* steps in which at least one game finished */
} ppenv_ppo_meter;

/* Bytes of the `partial` workspace: one ppenv_ppo_meter_partial per step and PPENV_PPO_METER_BLOCK envs (0 when h < 1 or num_envs < 1). */
size_t ppo_meter_partial_bytes(int32_t h, int32_t num_envs);

/* One horizon.  rew / done: [h, >= num_agents * num_envs] with row strides ld_rew / ld_done in elements (unit stride inside a row).
 * cur_reward [num_envs] f32, cur_len [num_envs] i32: the envs' running games, carried from call to call.  games_to_track >= 1,
 * num_agents 1 or 2.  partial: ppo_meter_partial_bytes(h, num_envs) bytes, 8-byte aligned (rewritten by every call). */
int ppo_meter_update(const float* rew, int64_t ld_rew, const int64_t* done, int64_t ld_done, int32_t h, int32_t num_envs, int32_t num_agents,
                     int64_t games_to_track, float* cur_reward, int32_t* cur_len, ppenv_ppo_meter* meter, ppenv_ppo_meter_partial* partial,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif
