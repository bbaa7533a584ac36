// ppenv_dr_device.h — per-env arithmetic of reset-time domain randomisation (include/ppenv_dr.h): the rule, the draw, the blend.
//
// PP_HD like ppenv_device.h: the HIP kernels in ppenv_dr.hip and the tests' host build (tests/csrc/dr_shim.cpp, g++) compile this
// text, and the two must agree BIT FOR BIT — a table column is drawn once per episode and then read by thousands of steps, so the
// device-versus-host tests compare tables exactly.  Hence: every product-and-sum that may fuse is written as fmaf(), everything else
// is compiled unfused (the pragma below; the host build passes -ffp-contract=off), the only operation beyond them is IEEE division (correctly
// rounded on both sides), and the square root, logarithm and sine / cosine of Box-Muller are iterations and polynomials of this
// file instead of libm on one side and the hardware's instructions on the other.  A redraw is rare (one per episode and
// env), so their ~60 instructions are off every step's path.
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_dr.h"

namespace pp {

PP_HD float dr_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
PP_HD float dr_bits_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
PP_HD uint32_t dr_float_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// sqrt x for a normal x > 0 (0 otherwise), within an ulp: the exponent-halving bit pattern (3.5 % off) and three Heron steps, each an
// IEEE division, sum and halving — the same bits wherever it runs.  (The device's own correctly rounded square root and the host's
// differ in the last bit on one input in six; measured on an MI355X against x86-64.)
PP_HD float dr_sqrt(float x) {
#pragma clang fp contract(off)
    if (!(x > 0.0f)) return 0.0f;
    float y = dr_bits_float((dr_float_bits(x) >> 1) + 0x1FBD1DF5u);
    y = 0.5f * (y + dr_div(x, y));
    y = 0.5f * (y + dr_div(x, y));
    y = 0.5f * (y + dr_div(x, y));
    return y;
}

// ln x for a normal x > 0: x = 2^e m, m in [sqrt(1/2), sqrt 2); ln m = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716: the series to
// s^11 leaves 5e-11 relative.
PP_HD float dr_log(float x) {
#pragma clang fp contract(off)
    const uint32_t bits = dr_float_bits(x);
    int32_t e = (int32_t)(bits >> 23) - 127;
    float m = dr_bits_float((bits & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421356f) { m = m * 0.5f; e += 1; }
    const float s = dr_div(m - 1.0f, m + 1.0f), z = s * s;
    float p = fmaf(z, 1.0f / 11.0f, 1.0f / 9.0f);
    p = fmaf(z, p, 1.0f / 7.0f);
    p = fmaf(z, p, 1.0f / 5.0f);
    p = fmaf(z, p, 1.0f / 3.0f);
    p = fmaf(z, p, 1.0f);
    return fmaf((float)e, 0.69314718f, 2.0f * s * p);
}
// cos and sin of 2 pi u, u in [0, 1) a multiple of 2^-24: quadrant q = round(4 u), r = 4 u - q in [-1/2, 1/2] (exact), Taylor series of
// the angle r pi / 2 in [-pi/4, pi/4] (to x^11 / x^10: 7e-12 / 1e-10), then the quadrant's rotation.
PP_HD void dr_cos_sin_rev(float u, float& c, float& s) {
#pragma clang fp contract(off)
    const float t = u * 4.0f;
    const int32_t q = (int32_t)(t + 0.5f);
    const float x = (t - (float)q) * 1.57079633f, x2 = x * x;
    float ps = fmaf(x2, -1.0f / 39916800.0f, 1.0f / 362880.0f);
    ps = fmaf(x2, ps, -1.0f / 5040.0f);
    ps = fmaf(x2, ps, 1.0f / 120.0f);
    ps = fmaf(x2, ps, -1.0f / 6.0f);
    const float sn = fmaf(x * x2, ps, x);
    float pc = fmaf(x2, -1.0f / 3628800.0f, 1.0f / 40320.0f);
    pc = fmaf(x2, pc, -1.0f / 720.0f);
    pc = fmaf(x2, pc, 1.0f / 24.0f);
    pc = fmaf(x2, pc, -0.5f);
    const float cs = fmaf(x2, pc, 1.0f);
    const int32_t k = q & 3;
    c = k == 0 ? cs : (k == 1 ? -sn : (k == 2 ? -cs : sn));
    s = k == 0 ? sn : (k == 1 ? cs : (k == 2 ? -sn : -cs));
}

PP_HD uint32_t dr_key(int32_t table_index, int32_t row) { return (uint32_t)table_index * (uint32_t)PPENV_DR_MAX_ROWS + (uint32_t)row; }

// The base variate of key k in redraw `draw` of global env gid: U[0, 1) or a unit normal (see ppenv_dr.h for the key and the pairing).
PP_HD float dr_base(uint64_t seed, uint32_t gid, uint32_t draw, uint32_t k, int32_t distribution) {
#pragma clang fp contract(off)
    const uint64_t sd = seed ^ PPENV_DR_SEED_SALT;
    if (distribution != PPENV_DR_GAUSSIAN) return rng_uniform(sd, gid, draw, k);
    const float u1 = rng_uniform(sd, gid, draw, k & ~1u), u2 = rng_uniform(sd, gid, draw, k | 1u);
    const float rad = dr_sqrt(-2.0f * dr_log(fmaxf(u1, 5.9604645e-8f)));     // u1 = 0 -> 2^-24: the largest radius a 24-bit draw can give
    float c, s;
    dr_cos_sin_rev(u2, c, s);
    return rad * ((k & 1u) ? s : c);
}

// Schedule weight at control step t (upstream VecTask.apply_randomizations as isaacgym_amd/vec_task.py restates it).
PP_HD float dr_schedule_weight(int32_t schedule, int32_t schedule_steps, int64_t t) {
    if (schedule == PPENV_DR_SCHED_LINEAR) {
        const int64_t c = t < 0 ? 0 : (t < schedule_steps ? t : schedule_steps);
        return dr_div((float)c, (float)schedule_steps);
    }
    if (schedule == PPENV_DR_SCHED_CONSTANT) return t > schedule_steps ? 1.0f : 0.0f;
    return 1.0f;
}

// base variate -> table value: `range` = (lo, hi) / (mu, sigma); a scaling blended towards 1, an additive term towards 0 by the weight.
// Each product and each sum rounds on its own, in the order torch evaluates `v * s + (1.0 - s)` on a float32 tensor.
PP_HD float dr_shape(float base, int32_t distribution, int32_t operation, float a, float b, float w) {
#pragma clang fp contract(off)
    const float scaled = distribution == PPENV_DR_GAUSSIAN ? base * b : base * (b - a);
    const float v = scaled + a;
    const float vw = v * w;
    const float r = operation == PPENV_DR_SCALING ? vw + (1.0f - w) : vw;
    // a zero is stored as +0 (a negative draw times a zero weight is -0 in IEEE and +0 under -fno-signed-zeros: the bits decide here)
    return (dr_float_bits(r) << 1) == 0u ? dr_bits_float(0u) : r;
}

PP_HD float dr_value(const ppenv_dr_entry& en, uint64_t seed, uint32_t gid, uint32_t draw, uint32_t k, int64_t t) {
    return dr_shape(dr_base(seed, gid, draw, k, en.distribution), en.distribution, en.operation, en.a, en.b,
                    dr_schedule_weight(en.schedule, en.schedule_steps, t));
}

// The rule of one control step for one env (TT:1025 + upstream's mask): advances randomize_buf, -> whether the env redraws now.
PP_HD bool dr_step_rule(bool first, int64_t reset, int32_t frequency, int64_t& randomize) {
    randomize += 1;
    if (first || (reset != 0 && randomize >= (int64_t)frequency)) { randomize = 0; return true; }
    return false;
}
// ... and for an env listed in reset_idx(env_ids): the listing stands for reset_buf != 0, no control step passes.
PP_HD bool dr_ids_rule(bool first, int32_t frequency, int64_t& randomize) {
    if (first || randomize >= (int64_t)frequency) { randomize = 0; return true; }
    return false;
}

// Redraw column e of every table of the plan.  Consecutive lanes = consecutive envs of one row: each store instruction is coalesced.
PP_HD void dr_redraw(const ppenv_dr_plan& P, int32_t e, uint32_t draw, int64_t t) {
    const uint32_t gid = (uint32_t)(P.env_id_offset + e);
    for (int32_t ti = 0; ti < P.num_tables; ++ti) {
        const ppenv_dr_entry& en = P.entry[ti];
        const float w = dr_schedule_weight(en.schedule, en.schedule_steps, t);
        for (int32_t r = 0; r < en.rows; ++r)
            en.table[(size_t)r * (size_t)P.num_envs + (size_t)e] =
                dr_shape(dr_base(P.seed, gid, draw, dr_key(ti, r), en.distribution), en.distribution, en.operation, en.a, en.b, w);
    }
}

// An env that redraws: count the redraw, rewrite its columns.  t = the control-step count the schedules see.
PP_HD void dr_redraw_env(const ppenv_dr_plan& P, int32_t e, int64_t t, int32_t* draws) {
    const int32_t d = draws[e];
    draws[e] = d + 1;
    dr_redraw(P, e, (uint32_t)d, t);
}
// One env of one control step (ppenv_dr_apply), `count` = control steps counted before this one; the schedules see count + 1.
PP_HD void dr_step_env(const ppenv_dr_plan& P, int32_t e, int64_t count, const int64_t* reset_buf, int64_t* randomize_buf, int32_t* draws) {
    int64_t rnd = randomize_buf[e];
    const bool fire = dr_step_rule(count == 0, reset_buf[(size_t)P.reset_rows * (size_t)e], P.frequency, rnd);
    randomize_buf[e] = rnd;
    if (fire) dr_redraw_env(P, e, count + 1, draws);
}
// One listed env of ppenv_dr_apply_ids.
PP_HD void dr_ids_env(const ppenv_dr_plan& P, int32_t e, int64_t count, int64_t* randomize_buf, int32_t* draws) {
    int64_t rnd = randomize_buf[e];
    if (!dr_ids_rule(count == 0, P.frequency, rnd)) return;
    randomize_buf[e] = rnd;
    dr_redraw_env(P, e, count, draws);
}

}  // namespace pp
