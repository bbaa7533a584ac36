/*
 * ppenv_play_group.h — C ABI of GROUPED episode accounting: ppenv_play.h's rule applied to G populations of envs at once, for playing
 * one checkpoint under G settings of the per-env physical parameters in a single pass (isaacgym_amd.play: Player(sweep=...)).
 *
 * Group g is envs [g * S, (g + 1) * S), S = envs_per_group, so the buffers hold G * S envs; with num_agents 2 it owns rows
 * [2 * g * S, 2 * (g + 1) * S) of `rew`, `done` and `cur_reward` (row num_agents * e + a is agent a of env e, as in ppenv_play.h).  Every
 * group has its own ppenv_play_totals, totals[g], and its own FREEZE: a call that finds totals[g].games >= games_num changes no word of
 * totals[g] and no cur_reward / cur_steps of group g's envs, bit for bit, while the other groups go on; `launches` counts per group.
 *
 * The rule: after any sequence of calls, totals[g] and group g's slices of cur_reward and cur_steps are BYTE FOR BYTE what
 * ppenv_play_reset / ppenv_play_accumulate leave when given S envs and group g's slices of `rew` and `done`.  It holds by construction:
 * ppenv_play.h's entries are the G = 1 case of these and run the same kernels, and nothing an env goes through depends on its group —
 * the sum order is chunks of PPENV_PLAY_BLOCK envs counted from the GROUP's first env (a ragged last chunk per group), the xor butterfly
 * within a wave, the four waves in order through LDS, one ppenv_play_partial per chunk; then per group lane l sums the group's partials
 * l, l + 64, ... in order, a butterfly, lane 0 adds the result to totals[g].
 *
 * Two launches per call, whatever G is.  play_rows_kernel: one workgroup per chunk, so a workgroup belongs to one group and the
 * freeze test is uniform in it; it reads totals[g].games and writes no word of the totals.  play_totals_kernel: one wave per
 * group; wave g reads and writes totals[g] and nobody else's.  No word read by one workgroup is written by another in the same launch;
 * no atomics; every sum has a fixed order, results are bitwise reproducible run to run.  The per-env arithmetic is
 * ppenv_play_device.h's.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the
 * message in ppenv_last_error().  Refused with PPENV_EINVAL before any device call: a NULL pointer, groups outside
 * 1..PP_PLAY_GROUP_MAX, envs_per_group <= 0, num_agents not 1 or 2, more than 2^31 - 1 rows, games_num < 1.
 */
#ifndef PPENV_PLAY_GROUP_H
#define PPENV_PLAY_GROUP_H

#include "ppenv_play.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_PLAY_GROUP_MAX 1024                        /* groups per call */

/* Bytes of the `partial` workspace: one ppenv_play_partial per PPENV_PLAY_BLOCK envs of a group, group after group (0 for sizes the
 * entries refuse). */
size_t pp_play_group_partial_bytes(int32_t envs_per_group, int32_t groups);

/* cur_reward [num_agents * groups * envs_per_group] f32 and cur_steps [groups * envs_per_group] i32 to zero; totals[0 .. groups) to zero
 * with reward_min = +inf, reward_max = -inf (both agents).  One launch. */
int pp_play_group_reset(int32_t envs_per_group, int32_t groups, int32_t num_agents, float* cur_reward, int32_t* cur_steps,
                        ppenv_play_totals* totals /* [groups] */, void* stream);

/* One control step of every group that is not frozen: ppenv_play_accumulate's rule on group g's envs and totals[g], for each g.
 * rew [num_agents * groups * envs_per_group] f32, done (same length) int64.  partial: pp_play_group_partial_bytes(envs_per_group,
 * groups) bytes, 8-byte aligned, owned by this state (rewritten by every call). */
int pp_play_group_accumulate(const float* rew, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents, int64_t games_num,
                             float* cur_reward, int32_t* cur_steps, ppenv_play_totals* totals /* [groups] */, ppenv_play_partial* partial,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif
