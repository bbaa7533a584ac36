// ppenv_serve_device.h — per-env arithmetic of the serve plan (include/ppenv_serve.h): the key, the draw, the store, the rule.
//
// PP_HD like ppenv_dr_device.h: the HIP kernels in ppenv_serve.hip and the tests' host build (tests/csrc/serve_shim.cpp, g++) compile this
// text and must agree BIT FOR BIT — the buffer it fills is consumed by a reset as is.  Both sides are compiled with -ffp-contract=off:
// every product and sum below, and those of serve_from_draws / sincos_small as instantiated here, round one by one.
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_serve.h"

namespace pp {

PP_HD bool serve_finite(float f) { uint32_t b; memcpy(&b, &f, 4); return (b & 0x7F800000u) != 0x7F800000u; }   // (whatever -ffinite-math-only says)

// 0 when the plan and its cells (host memory) are acceptable, else which rule of pp_serve_plan_upload they break (1 .. 7).
PP_HD int serve_plan_invalid(const pp_serve_plan& P, const pp_serve_cell* cells) {
    if (P.num_envs < 1 || P.groups < 1 || P.envs_per_group < 1 || (int64_t)P.groups * (int64_t)P.envs_per_group != (int64_t)P.num_envs) return 1;
    if (P.env_id_offset < 0 || (P.paired != 0 && P.paired != 1)) return 2;
    if (P.form != PPENV_VARIANT_T3 && P.form != PPENV_VARIANT_TT && P.form != PPENV_VARIANT_TN && P.form != PPENV_VARIANT_T4) return 3;
    if (P.layout != PP_SERVE_LAYOUT_SOA3 && P.layout != PP_SERVE_LAYOUT_AOS5) return 4;
    if (P.reset_rows != 1 && P.reset_rows != 2) return 5;
    if (!cells) return 6;
    for (int32_t g = 0; g < P.groups; ++g) {
        const pp_serve_cell& c = cells[g];
        const float v[10] = {c.speed_lo, c.speed_hi, c.tilt_lo_deg, c.tilt_hi_deg, c.tilt_z_lo_deg, c.tilt_z_hi_deg, c.ball_y_lo, c.ball_y_hi, c.ball_z_lo, c.ball_z_hi};
        for (int k = 0; k < 10; ++k)
            if (!serve_finite(v[k])) return 6;
        for (int k = 0; k < 10; k += 2)
            if (v[k] > v[k + 1]) return 6;
        for (int k = 2; k < 6; ++k)
            if (v[k] > PP_SERVE_MAX_TILT_DEG || v[k] < -PP_SERVE_MAX_TILT_DEG) return 7;
    }
    return 0;
}

PP_HD uint32_t serve_key(const pp_serve_plan& P, int32_t e) {
    return P.paired ? (uint32_t)(e % P.envs_per_group) : (uint32_t)(P.env_id_offset + e);
}

struct ServeRow { float y, z; V3 v; };

// serve(e, j) of the plan
PP_HD ServeRow serve_draw(const pp_serve_plan& P, int32_t e, uint32_t j) {
    const pp_serve_cell& c = P.cells[e / P.envs_per_group];
    const uint32_t key = serve_key(P, e);
    const float speed = c.speed_lo + (c.speed_hi - c.speed_lo) * rng_uniform(P.seed, key, j, 0u);
    const float tilt = c.tilt_lo_deg + (c.tilt_hi_deg - c.tilt_lo_deg) * rng_uniform(P.seed, key, j, 1u);
    const float tilt_z = P.form == PPENV_VARIANT_T3 ? 0.0f : c.tilt_z_lo_deg + (c.tilt_z_hi_deg - c.tilt_z_lo_deg) * rng_uniform(P.seed, key, j, 2u);
    ServeRow r;
    r.y = r.z = 0.0f;
    if (P.layout == PP_SERVE_LAYOUT_AOS5) {
        r.y = c.ball_y_lo + (c.ball_y_hi - c.ball_y_lo) * rng_uniform(P.seed, key, j, 3u);
        r.z = c.ball_z_lo + (c.ball_z_hi - c.ball_z_lo) * rng_uniform(P.seed, key, j, 4u);
    }
    r.v = serve_from_draws(P.form, speed, tilt, tilt_z);
    return r;
}

// Layout 0: consecutive lanes = consecutive floats of one component.  Layout 1: one 20-byte row per (rare) resetting lane, stored as is.
PP_HD void serve_store(const pp_serve_plan& P, int32_t e, const ServeRow& r, float* out) {
    if (P.layout == PP_SERVE_LAYOUT_AOS5) {
        float* o = out + 5 * (size_t)e;
        o[0] = r.y; o[1] = r.z; o[2] = r.v.x; o[3] = r.v.y; o[4] = r.v.z;
    } else {
        const size_t n = (size_t)P.num_envs;
        out[e] = r.v.x; out[n + e] = r.v.y; out[2 * n + e] = r.v.z;
    }
}

// pp_serve_fill's env
PP_HD void serve_fill_env(const pp_serve_plan& P, int32_t e, float* out, const uint32_t* count) { serve_store(P, e, serve_draw(P, e, count[e]), out); }

// An env that has consumed its serve: count it, put the next one in its place.
PP_HD void serve_advance_env(const pp_serve_plan& P, int32_t e, float* out, uint32_t* count) {
    const uint32_t j = count[e] + 1u;
    count[e] = j;
    serve_store(P, e, serve_draw(P, e, j), out);
}

// pp_serve_apply's env: all 64 bits of the reset word decide
PP_HD void serve_step_env(const pp_serve_plan& P, int32_t e, const int64_t* reset_buf, float* out, uint32_t* count) {
    if (reset_buf[(size_t)P.reset_rows * (size_t)e] != 0) serve_advance_env(P, e, out, count);
}

}  // namespace pp
