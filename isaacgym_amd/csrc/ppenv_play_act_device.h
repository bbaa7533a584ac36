// ppenv_play_act_device.h — per-element arithmetic of the actuator usage accounting (include/ppenv_play_act.h): one env's sample, the
// fold of its running episode into a partial, the merge of two partials, the totals' update.
//
// PP_HD like ppenv_play_pair_device.h: the HIP kernels in ppenv_play_act.hip and the tests' host build (tests/csrc/play_act_shim.cpp,
// g++) compile this text, and the two must agree BYTE FOR BYTE — the running state, and the totals when the host sums in the kernels'
// order.  Both sides are compiled with -ffp-contract=off (t * t and t * v are rounded before they are added or compared), with signed
// zeros, and without -ffinite-math-only (max_exc starts at -inf).
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_play_act.h"

namespace pp {

enum { ACT_ABS_TAU = 0, ACT_TAU_SQ, ACT_POWER, ACT_MAX_TAU, ACT_MAX_VEL, ACT_MAX_EXC, ACT_C_EFFORT, ACT_C_VEL, ACT_C_LIMIT, ACT_C_CLIP };

PP_HD float act_inf() { return __builtin_huge_valf(); }
PP_HD float act_abs(float x) { return __builtin_fabsf(x); }
PP_HD float act_max(float a, float b) { return b > a ? b : a; }

// word of env e in field f of dof d: plane 1 + f * D + d of N words each; plane 0 is n
PP_HD size_t act_word(int32_t f, int32_t d, int32_t num_dofs, int64_t num_envs, int64_t e) {
    return (size_t)(1 + f * num_dofs + d) * (size_t)num_envs + (size_t)e;
}

PP_HD float act_in(const pp_play_act_input& in, int64_t e, int32_t d) { return in.p[e * in.env_stride + (int64_t)d * in.dof_stride]; }

PP_HD void act_group_clear(pp_play_act_group& p) {
    p.games = p.samples = p.launches = 0;
    p.energy = p.energy_sq = 0.0;
}

PP_HD void act_joint_clear(pp_play_act_joint& p) {
    p.c_effort = p.c_vel = p.c_limit = p.c_clip = 0;
    p.abs_tau = p.tau_sq = p.power = 0.0;
    p.max_abs_tau = p.max_abs_vel = 0.0f;
    p.max_exc = -act_inf();
    p.reserved = 0.0f;
}

// into += from (the games of two disjoint sets of envs); `launches` is the totals' own
PP_HD void act_group_merge(pp_play_act_group& into, const pp_play_act_group& from) {
    into.games += from.games;
    into.samples += from.samples;
    into.energy += from.energy;
    into.energy_sq += from.energy_sq;
}

PP_HD void act_joint_merge(pp_play_act_joint& into, const pp_play_act_joint& from) {
    into.c_effort += from.c_effort;
    into.c_vel += from.c_vel;
    into.c_limit += from.c_limit;
    into.c_clip += from.c_clip;
    into.abs_tau += from.abs_tau;
    into.tau_sq += from.tau_sq;
    into.power += from.power;
    into.max_abs_tau = act_max(into.max_abs_tau, from.max_abs_tau);
    into.max_abs_vel = act_max(into.max_abs_vel, from.max_abs_vel);
    into.max_exc = act_max(into.max_exc, from.max_exc);
}

// The freeze: the launch changes nothing of a group once games_num games are counted.
PP_HD bool act_frozen(int64_t games, int64_t games_num) { return games >= games_num; }

// Memory first, arithmetic second: a lane walks its env's dofs alone, and a loop that loads, computes and stores one dof at a time pays
// one memory round trip per dof (27 of them on the 27-dof task).  The dofs are taken ACT_BATCH at a time — every load of the batch is
// issued before the first value is used — which changes when a word is read, never what is computed from it.
enum { ACT_BATCH = 9 };

// A sample of env e (done[A * e] == 0): every dof in order, then n += 1.  fp32, each operation rounded on its own.
PP_HD void act_sample(int64_t e, int64_t num_envs, int32_t num_dofs, const pp_play_act_inputs& in, const pp_play_act_limit* limits,
                      const pp_play_act_thresholds& thr, void* state) {
    float* sf = (float*)state;
    int32_t* si = (int32_t*)state;
    const int32_t n = si[e];
    const size_t step = (size_t)num_dofs * (size_t)num_envs;   // field f of a dof is `step` words after field f - 1
    for (int32_t d0 = 0; d0 < num_dofs; d0 += ACT_BATCH) {
        float t[ACT_BATCH], v[ACT_BATCH], x[ACT_BATCH], a[ACT_BATCH], run[ACT_BATCH][ACT_C_EFFORT];
        int32_t cnt[ACT_BATCH][PP_PLAY_ACT_FIELDS - ACT_C_EFFORT];
#pragma unroll
        for (int32_t k = 0; k < ACT_BATCH; ++k) {                // the loads; past the last dof the last dof's again (never used)
            const int32_t d = d0 + k < num_dofs ? d0 + k : num_dofs - 1;
            const size_t w0 = act_word(0, d, num_dofs, num_envs, e);
            t[k] = act_in(in.tau, e, d);
            v[k] = act_in(in.qd, e, d);
            x[k] = act_in(in.q, e, d);
            a[k] = in.action.p ? act_in(in.action, e, d) : 0.0f;
#pragma unroll
            for (int32_t f = 0; f < ACT_C_EFFORT; ++f) run[k][f] = sf[w0 + (size_t)f * step];
#pragma unroll
            for (int32_t f = ACT_C_EFFORT; f < PP_PLAY_ACT_FIELDS; ++f) cnt[k][f - ACT_C_EFFORT] = si[w0 + (size_t)f * step];
        }
#pragma unroll
        for (int32_t k = 0; k < ACT_BATCH; ++k) {
            const int32_t d = d0 + k;
            if (d >= num_dofs) break;
            const pp_play_act_limit lim = limits[d];
            const size_t w0 = act_word(0, d, num_dofs, num_envs, e);
            const float at = act_abs(t[k]), av = act_abs(v[k]);
            const float tt = t[k] * t[k], tv = t[k] * v[k];
            const float lo = lim.lower - x[k], hi = x[k] - lim.upper;
            const float exc = act_max(lo, hi);
            sf[w0 + ACT_ABS_TAU * step] = run[k][ACT_ABS_TAU] + at;
            sf[w0 + ACT_TAU_SQ * step] = run[k][ACT_TAU_SQ] + tt;
            sf[w0 + ACT_POWER * step] = run[k][ACT_POWER] + act_abs(tv);
            sf[w0 + ACT_MAX_TAU * step] = act_max(run[k][ACT_MAX_TAU], at);
            sf[w0 + ACT_MAX_VEL * step] = act_max(run[k][ACT_MAX_VEL], av);
            sf[w0 + ACT_MAX_EXC * step] = n == 0 ? exc : act_max(run[k][ACT_MAX_EXC], exc);
            const float effort_at = thr.effort_frac * lim.effort, vel_at = thr.vel_frac * lim.vel_limit;
            si[w0 + ACT_C_EFFORT * step] = cnt[k][0] + (at >= effort_at ? 1 : 0);
            si[w0 + ACT_C_VEL * step] = cnt[k][1] + (av >= vel_at ? 1 : 0);
            si[w0 + ACT_C_LIMIT * step] = cnt[k][2] + (exc >= -thr.limit_margin ? 1 : 0);
            if (in.action.p) si[w0 + ACT_C_CLIP * step] = cnt[k][3] + (act_abs(a[k]) >= thr.action_clip ? 1 : 0);
        }
    }
    si[e] = n + 1;
}

// The fold of env e (done[A * e] != 0), first half: the finished game's n and energy into `acc`, n to zero.  -> the game's n, which
// act_fold_joint needs.  The dofs' words are still the game's: act_fold_zero clears them.
PP_HD int32_t act_fold_env(int64_t e, int64_t num_envs, int32_t num_dofs, void* state, pp_play_act_group& acc) {
    const float* sf = (const float*)state;
    int32_t* si = (int32_t*)state;
    const int32_t n = si[e];
    float energy = 0.0f;
    for (int32_t d0 = 0; d0 < num_dofs; d0 += ACT_BATCH) {
        float pw[ACT_BATCH];
#pragma unroll
        for (int32_t k = 0; k < ACT_BATCH; ++k) pw[k] = sf[act_word(ACT_POWER, d0 + k < num_dofs ? d0 + k : num_dofs - 1, num_dofs, num_envs, e)];
#pragma unroll
        for (int32_t k = 0; k < ACT_BATCH; ++k)
            if (d0 + k < num_dofs) energy = energy + pw[k];       // d ascending
    }
    const double ed = (double)energy;
    acc.games += 1;
    acc.samples += (int64_t)n;
    acc.energy += ed;
    acc.energy_sq += ed * ed;                                  // exact: a 24-bit significand squared
    si[e] = 0;
    return n;
}

// ... second half, once per dof, in three steps so that a caller can have the next dofs' words on their way while it sums these:
// the ten running words of dof d
struct act_joint_words {
    float f[ACT_C_EFFORT];
    int32_t c[PP_PLAY_ACT_FIELDS - ACT_C_EFFORT];
};

PP_HD void act_fold_load(int64_t e, int64_t num_envs, int32_t num_dofs, int32_t d, const void* state, act_joint_words& w) {
    const float* sf = (const float*)state;
    const int32_t* si = (const int32_t*)state;
    const size_t w0 = act_word(0, d, num_dofs, num_envs, e), step = (size_t)num_dofs * (size_t)num_envs;
#pragma unroll
    for (int32_t f = 0; f < ACT_C_EFFORT; ++f) w.f[f] = sf[w0 + (size_t)f * step];
#pragma unroll
    for (int32_t f = ACT_C_EFFORT; f < PP_PLAY_ACT_FIELDS; ++f) w.c[f - ACT_C_EFFORT] = si[w0 + (size_t)f * step];
}

// ... into `acc` (n: the game's samples, act_fold_env's) ...
PP_HD void act_fold_joint(const act_joint_words& w, int32_t n, pp_play_act_joint& acc) {
    acc.abs_tau += (double)w.f[ACT_ABS_TAU];
    acc.tau_sq += (double)w.f[ACT_TAU_SQ];
    acc.power += (double)w.f[ACT_POWER];
    acc.max_abs_tau = act_max(acc.max_abs_tau, w.f[ACT_MAX_TAU]);
    acc.max_abs_vel = act_max(acc.max_abs_vel, w.f[ACT_MAX_VEL]);
    if (n > 0) acc.max_exc = act_max(acc.max_exc, w.f[ACT_MAX_EXC]);
    acc.c_effort += (int64_t)w.c[0];
    acc.c_vel += (int64_t)w.c[1];
    acc.c_limit += (int64_t)w.c[2];
    acc.c_clip += (int64_t)w.c[3];
}

// ... and to zero, every word through its own type.
PP_HD void act_fold_zero(int64_t e, int64_t num_envs, int32_t num_dofs, int32_t d, void* state) {
    float* sf = (float*)state;
    int32_t* si = (int32_t*)state;
    const size_t w0 = act_word(0, d, num_dofs, num_envs, e), step = (size_t)num_dofs * (size_t)num_envs;
#pragma unroll
    for (int32_t f = 0; f < ACT_C_EFFORT; ++f) sf[w0 + (size_t)f * step] = 0.0f;
#pragma unroll
    for (int32_t f = ACT_C_EFFORT; f < PP_PLAY_ACT_FIELDS; ++f) si[w0 + (size_t)f * step] = 0;
}

// totals += the launch's games; one more control step counted
PP_HD void act_group_add(pp_play_act_group& t, const pp_play_act_group& p) {
    act_group_merge(t, p);
    t.launches += 1;
}

}  // namespace pp
