/*
 * ppenv_play_pair.h — C ABI of PAIRED episode statistics: for G groups of envs that are served the same balls (isaacgym_amd.play:
 * Sweep(paired=True)), the return and the length of the first M episodes of EVERY env, and from them, per cell, the sums of the paired
 * difference `return(cell, env i, episode m) - return(baseline, env i, episode m)` (isaacgym_amd.play: Player(paired_diff=True)).
 *
 * ppenv_play_group.h's totals cannot give that difference: they keep sums per group, not a return per (i, m), and they count the first
 * games_num games to FINISH, a set that favours short episodes and differs from cell to cell.  Here a pair is (env i, episode m) with
 * m < M, the same set in every cell.
 *
 * Layout as in ppenv_play_group.h: group g is envs [g * S, (g + 1) * S), S = envs_per_group; row num_agents * e + a of `rew`, `done`
 * and `cur_reward` is agent a of env e (num_agents 1 or 2); env e has finished a game when the whole 64-bit word
 * done[num_agents * e] != 0.  State, allocated by the caller (pp_play_pair_*_bytes):
 *     cur_reward [A * G * S] f32, cur_steps [G * S] i32     the running episode, ppenv_play_accumulate's `cr += r` in the same step order
 *     count      [G * S]     i32                            episodes of the env in the table, 0 .. M
 *     ret        [G][S][M][A] f32                           return of episode m of env i of group g, per agent; quiet NaN while not played
 *     len        [G][S][M]   i32                            its length in control steps; 0 while not played
 * There is NO FREEZE: an env's episodes after its M-th change nothing but its running values, so the table's final content does not
 * depend on how long the caller goes on stepping.
 *
 * pp_play_pair_reduce sums, for cell g with b = baseline[g], over the pairs (i, m) with m < min(count[g][i], count[b][i]) — the
 * episodes BOTH have played — in fp64 and in a FIXED order: pairs are numbered p = i * M + m; lane l of the cell's one workgroup of
 * PPENV_PLAY_BLOCK lanes takes p = l, l + PPENV_PLAY_BLOCK, ... in order; an xor butterfly within each wave; the waves in order through
 * LDS (the shape of play_rows_kernel).  out[g] is OVERWRITTEN: the entry is idempotent and is meant for polls, not for every step.
 *
 * No atomics, no word read by one workgroup and written by another in the same launch; results are bitwise reproducible run to run and
 * equal the host build of the per-element header (isaacgym_amd/csrc/ppenv_play_pair_device.h) summed in that order.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the message
 * in ppenv_last_error().  Refused with PPENV_EINVAL before any device call: a NULL pointer, groups outside 1..PP_PLAY_GROUP_MAX,
 * envs_per_group < 1, num_agents not 1 or 2, episodes < 1, more than 2^31 - 1 table entries (G * S * M * A).
 */
#ifndef PPENV_PLAY_PAIR_H
#define PPENV_PLAY_PAIR_H

#include "ppenv_play_group.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The paired sums of one cell against its baseline. */
typedef struct pp_play_pair_totals {
    int64_t pairs;                                    /* pairs (i, m) both cells have played; -1: baseline[g] was outside 0 .. G-1 */
    int64_t steps_diff;                               /* sum of len(cell) - len(baseline) */
    double diff[PPENV_PLAY_MAX_AGENTS];               /* sum of d = (double) ret(cell) - (double) ret(baseline), per agent */
    double diff_sq[PPENV_PLAY_MAX_AGENTS];            /* sum of d * d (rounded once, then added) */
    double cell[PPENV_PLAY_MAX_AGENTS];               /* sum of ret(cell) over the pairs */
    double base[PPENV_PLAY_MAX_AGENTS];               /* sum of ret(baseline) over the pairs */
} pp_play_pair_totals;

/* Bytes of `ret` (G * S * M * A floats) and of `len` (G * S * M int32); 0 for sizes the entries refuse. */
size_t pp_play_pair_ret_bytes(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes);
size_t pp_play_pair_len_bytes(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes);

/* cur_reward, cur_steps, count and len to zero, ret to quiet NaN (0x7fc00000).  One launch. */
int pp_play_pair_reset(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes, float* cur_reward, int32_t* cur_steps,
                       int32_t* count, float* ret, int32_t* len, void* stream);

/* One control step, after the env step that wrote rew [A * G * S] f32 and done (same length) int64.  Per env e, with m = count[e]:
 *     cur_steps[e] += 1;  cur_reward[r] = fl32(cur_reward[r] + rew[r]) for its rows r
 *     if done[A * e] != 0:  if m < M: ret[e][m][a] = cur_reward[r], len[e][m] = cur_steps[e];
 *                           count[e] = min(m + 1, M);  cur_reward[r] = 0, cur_steps[e] = 0
 * One launch, one lane per env. */
int pp_play_pair_record(const float* rew, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes,
                        float* cur_reward, int32_t* cur_steps, int32_t* count, float* ret, int32_t* len, void* stream);

/* out[g] = the paired sums of cell g against cell baseline[g], for every g (see above).  baseline: int32 [groups] on the device, each in
 * 0 .. groups - 1 (the caller checks before the upload; a value outside reads nothing and gives out[g] = {pairs = -1, zeros}).  One
 * launch, one workgroup per cell; reads the state, writes out[0 .. groups) only. */
int pp_play_pair_reduce(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes, const int32_t* baseline,
                        const int32_t* count, const float* ret, const int32_t* len, pp_play_pair_totals* out /* [groups] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif
