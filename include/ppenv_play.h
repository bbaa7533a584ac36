/*
 * ppenv_play.h — C ABI of episode accounting for playing a checkpoint (the reference's `test=true`, train.py:210-215: rl_games'
 * BasePlayer.run — restated from its published code, rl_games is absent offline: parity unpinned).
 *
 * rl_games' player keeps a running return `cr` and a running length `steps` per row, reads `done.nonzero()` ON THE HOST every step,
 * adds the finished rows' values to its sums, zeroes them, and leaves its loop after the step in which games_played >= n_games.
 * Here the same accounting is one entry per control step on the device, ppenv_play_accumulate, and the host reads the totals only now
 * and then to decide when to stop.  That is safe because of the FREEZE: a call that finds totals.games >= games_num changes nothing,
 * bit for bit — so the totals after any number of further steps are those of the step the host-synchronised loop would have
 * stopped at (all envs that finish in that step are counted: games may exceed games_num by at most num_envs - 1).
 *
 * Row num_agents * e + a of `rew`, `done` and `cur_reward` belongs to agent a of env e (num_agents 1, or 2 for the 4-actor task); an
 * env has finished a game when done[num_agents * e] != 0 — agent 0's row, rl_games' all_done_indices[::num_agents]; the whole
 * 64-bit word is tested (2 and 2^32 are done).
 *
 * Two launches per call, the shape of ppenv_ppo_loss_grad.  play_rows_kernel: lane e owns env e, 256 envs per workgroup; it
 * advances cur_reward / cur_steps, and each workgroup writes ONE ppenv_play_partial (its finished games, summed by wave shuffles and LDS
 * in a fixed order).  play_totals_kernel: one wave sums the partials in a fixed order and adds them to the totals.  Both read
 * totals.games for the freeze; only the second writes the totals — no word a workgroup reads is written by another workgroup in the
 * same launch.  No atomics: every sum has a fixed order, results are bitwise reproducible run to run.
 * Sums across games are fp64 (a game's return itself is fp32, rl_games' `cr += r` in step order).
 *
 * These entries are the G = 1 case of ppenv_play_group.h's (one group of num_envs envs, totals[0] = *totals) and run the same kernels;
 * they keep their own argument validation and error texts.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the
 * message in ppenv_last_error().
 */
#ifndef PPENV_PLAY_H
#define PPENV_PLAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPENV_PLAY_MAX_AGENTS 2
#define PPENV_PLAY_BLOCK 256                          /* envs per workgroup = envs per partial */

/* The finished games of a set of envs: a workgroup's in one launch (workspace), and the layout the totals continue. */
typedef struct ppenv_play_partial {
    int64_t games;                                    /* envs that finished a game */
    int64_t steps;                                    /* sum of their lengths in control steps */
    double reward[PPENV_PLAY_MAX_AGENTS];             /* sum of the games' returns, per agent */
    double reward_sq[PPENV_PLAY_MAX_AGENTS];          /* sum of their squares */
    float reward_min[PPENV_PLAY_MAX_AGENTS];          /* +inf while empty */
    float reward_max[PPENV_PLAY_MAX_AGENTS];          /* -inf while empty */
} ppenv_play_partial;

typedef struct ppenv_play_totals {
    int64_t games;
    int64_t steps;
    int64_t launches;                                 /* control steps accumulated while not frozen */
    double reward[PPENV_PLAY_MAX_AGENTS];
    double reward_sq[PPENV_PLAY_MAX_AGENTS];
    float reward_min[PPENV_PLAY_MAX_AGENTS];
    float reward_max[PPENV_PLAY_MAX_AGENTS];
} ppenv_play_totals;

/* Bytes of the `partial` workspace for num_envs envs: one ppenv_play_partial per PPENV_PLAY_BLOCK envs (0 when num_envs <= 0). */
size_t ppenv_play_partial_bytes(int32_t num_envs);

/* cur_reward [num_agents * num_envs] f32 and cur_steps [num_envs] i32 to zero; *totals to zero with reward_min = +inf,
 * reward_max = -inf (both agents).  One launch. */
int ppenv_play_reset(int32_t num_envs, int32_t num_agents, float* cur_reward, int32_t* cur_steps, ppenv_play_totals* totals, void* stream);

/* One control step, after the env step that wrote rew [num_agents * num_envs] f32 and done [num_agents * num_envs] int64
 * (VecTask.step's rew_buf / reset_buf, or a [rows] slice of a collector's [H, rows] buffers).  If totals->games >= games_num when the
 * call's launches start: nothing changes.  Otherwise, per env e:
 *     cur_steps[e] += 1;  cur_reward[r] = fl32(cur_reward[r] + rew[r]) for its rows r
 *     if done[num_agents * e] != 0:  games += 1, steps += cur_steps[e], per agent reward += (double) cur_reward[r],
 *         reward_sq += (double) cur_reward[r]^2, min / max updated;  cur_reward[r] = 0, cur_steps[e] = 0
 * and launches += 1.  partial: ppenv_play_partial_bytes(num_envs) bytes, 8-byte aligned, owned by this state (rewritten by every call). */
int ppenv_play_accumulate(const float* rew, const int64_t* done, int32_t num_envs, int32_t num_agents, int64_t games_num, float* cur_reward,
                          int32_t* cur_steps, ppenv_play_totals* totals, ppenv_play_partial* partial, void* stream);

#ifdef __cplusplus
}
#endif

#endif
