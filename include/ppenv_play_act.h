/*
 * ppenv_play_act.h — C ABI of the ACTUATOR USAGE accounting of a played checkpoint: per joint, how hard the policy drives the robot —
 * torque against the effort limit, speed against the velocity limit, position against the joint limits, mechanical power, raw actions
 * beyond clipActions — summed on the device over the games ppenv_play_group.h counts, per group of envs (isaacgym_amd.play:
 * Player(actuators=True), one report per sweep cell).
 *
 * Layout as in ppenv_play_group.h: group g is envs [g * S, (g + 1) * S), S = envs_per_group; env e has finished a game when the whole
 * 64-bit word done[num_agents * e] != 0 (num_agents 1 or 2).  An env has D = num_dofs joints (7; 14 on the 4-actor task, agent a's being
 * 7a .. 7a + 6; 27).  Every input is a float array with two strides in ELEMENTS: value (e, d) is p[e * env_stride + d * dof_stride] — the
 * 7-dof SoA [D][N] is (1, N), the 27-dof AoS dof_states [N, 27, 2] is (54, 2) from &dof_states[0][0][0] (positions) or [0][0][1]
 * (velocities), dof_force [N, 27] and an action tensor [A * N, D / A] are (D, 1).
 *
 * RUNNING STATE per env, `state`: 1 + 10 * D planes of N = G * S 32-bit words, plane-major (word `plane * N + e`), all zero after
 * pp_play_act_reset:
 *     plane 0                      n            i32   samples of the running episode
 *     plane 1 + f * D + d          field f of dof d:
 *         f = 0 abs_tau, 1 tau_sq, 2 power                    f32 sums
 *         f = 3 max_abs_tau, 4 max_abs_vel, 5 max_exc         f32 maxima (max_exc is meaningful while n > 0 only)
 *         f = 6 c_effort, 7 c_vel, 8 c_limit, 9 c_clip        i32 counters
 *
 * THE RULE, per call and per env e of a group that is not frozen:
 *   done[A * e] == 0: a SAMPLE.  For d = 0 .. D - 1 in order, with t = tau, v = qd, x = q, a = action, every operation in fp32 and
 *   rounded on its own (no contraction):
 *       abs_tau += |t|;  tau_sq += t * t;  power += |t * v|                (the products rounded first, as the reward's power term)
 *       max_abs_tau = max(max_abs_tau, |t|);  max_abs_vel = max(max_abs_vel, |v|)
 *       exc = max(lower - x, x - upper);  max_exc = n == 0 ? exc : max(max_exc, exc)           (positive: beyond the limit)
 *       c_effort += |t| >= effort_frac * effort;  c_vel += |v| >= vel_frac * vel_limit
 *       c_limit  += exc >= -limit_margin;         c_clip += |a| >= action_clip                 (0 when `action` is NULL)
 *   then n += 1.
 *   done[A * e] != 0: NO sample — the state the step left is already the next episode's post-reset state — and a FOLD: the running
 *   episode goes into the group's totals (joint sums as fp64, counters as int64, maxima merged; max_exc only when n > 0), games += 1,
 *   samples += n, E = sum over d ascending of power[d] in fp32, energy += (double) E, energy_sq += (double) E * (double) E; then the
 *   env's running words are zeroed.  A game of `length` control steps contributes length - 1 samples.
 *   launches += 1 per group and call.
 * FREEZE: a call that finds group[g].games >= games_num changes no word of group[g], of joint[g * D ..], or of the running state of
 * group g's envs.  The counter is this accounting's own; it counts the done words pp_play_group_accumulate counts, under the same rule.
 *
 * Two launches per call, the shape of play_rows_kernel / play_totals_kernel: chunks of PPENV_PLAY_BLOCK envs counted from the group's
 * first env, one lane per env, one partial (a pp_play_act_group and D pp_play_act_joint) per chunk — an xor butterfly within a wave (strides 1 up to 32), the
 * waves in order through LDS; a workgroup in which no env finished skips the reductions and writes the empty partial (a uniform
 * branch).  Then one workgroup per group, a wave per three dofs: lane l sums the partials l, l + 64, ... in order, a butterfly, one lane
 * adds the result to the totals (group[g] after a barrier: every wave tests its games first).  No atomics, no word read by one workgroup and written by another in the same launch; every sum has a fixed order: results
 * are bitwise reproducible run to run and equal, byte for byte, the host build of isaacgym_amd/csrc/ppenv_play_act_device.h summed in
 * that order.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the message
 * in ppenv_last_error().  Refused with PPENV_EINVAL before any device call: a NULL pointer (the action's excepted), num_dofs outside
 * 1..PP_PLAY_ACT_MAX_DOF or no multiple of num_agents, groups outside 1..PP_PLAY_GROUP_MAX, envs_per_group <= 0, num_agents not 1 or 2,
 * more than 2^31 - 1 rows, games_num < 1.
 */
#ifndef PPENV_PLAY_ACT_H
#define PPENV_PLAY_ACT_H

#include "ppenv_play_group.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_PLAY_ACT_MAX_DOF 32
#define PP_PLAY_ACT_FIELDS 10                         /* state planes per dof */

typedef struct pp_play_act_limit {                    /* one joint, the numbers the step kernels run with */
    float lower, upper;                               /* rad */
    float effort;                                     /* N m */
    float vel_limit;                                  /* rad / s */
} pp_play_act_limit;

typedef struct pp_play_act_thresholds {
    float effort_frac;                                /* at the effort limit: |tau| >= effort_frac * effort */
    float vel_frac;                                   /* at the velocity limit: |qd| >= vel_frac * vel_limit */
    float limit_margin;                               /* at a position limit: within limit_margin rad of it, or beyond */
    float action_clip;                                /* raw action at the clamp: |a| >= action_clip */
} pp_play_act_thresholds;

typedef struct pp_play_act_input {                    /* value (e, d) = p[e * env_stride + d * dof_stride] */
    const float* p;
    int64_t env_stride, dof_stride;
} pp_play_act_input;

typedef struct pp_play_act_inputs {
    pp_play_act_input q, qd, tau, action;             /* action.p may be NULL */
} pp_play_act_inputs;

typedef struct pp_play_act_group {                    /* per group; also the per-chunk partial (launches unused there) */
    int64_t games;
    int64_t samples;
    int64_t launches;                                 /* control steps accumulated while not frozen */
    double energy;                                    /* sum over games of E = sum_d sum_samples |tau * qd|   [W; x control dt = J] */
    double energy_sq;
} pp_play_act_group;

typedef struct pp_play_act_joint {                    /* per (group, dof); also the per-chunk partial */
    int64_t c_effort, c_vel, c_limit, c_clip;
    double abs_tau, tau_sq, power;
    float max_abs_tau, max_abs_vel;                   /* 0 while empty */
    float max_exc;                                    /* -inf while empty */
    float reserved;                                   /* 0 */
} pp_play_act_joint;

/* Bytes of `state` (4 * (1 + 10 * D) * G * S) and of the `partial` workspace (per chunk one pp_play_act_group, then per chunk D
 * pp_play_act_joint); 0 for sizes the entries refuse. */
size_t pp_play_act_state_bytes(int32_t envs_per_group, int32_t groups, int32_t num_dofs);
size_t pp_play_act_partial_bytes(int32_t envs_per_group, int32_t groups, int32_t num_dofs);

/* state to zero; group[0 .. G) and joint[0 .. G * D) to zero with max_exc = -inf.  One launch. */
int pp_play_act_reset(int32_t envs_per_group, int32_t groups, int32_t num_dofs, void* state, pp_play_act_group* group /* [G] */,
                      pp_play_act_joint* joint /* [G * D] */, void* stream);

/* One control step, after the env step that wrote the inputs and done [A * G * S] int64.  `in` and `thresholds` are HOST structs read
 * during the call; limits [D] is on the device.  partial: pp_play_act_partial_bytes bytes, 8-byte aligned, rewritten by every call. */
int pp_play_act_accumulate(const pp_play_act_inputs* in, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents,
                           int32_t num_dofs, int64_t games_num, const pp_play_act_limit* limits, const pp_play_act_thresholds* thresholds,
                           void* state, pp_play_act_group* group, pp_play_act_joint* joint, void* partial, void* stream);

#ifdef __cplusplus
}
#endif

#endif
