// ppenv_serve_curric_device.h — per-env and per-bin arithmetic of the serve curriculum (include/ppenv_serve_curric.h has the rule).
//
// The reference has no serve curriculum: the rule is this project's own specification, unpinned by any oracle.
//
// PP_HD like ppenv_serve_device.h, whose serve_draw and serve_store it calls through a one-group view of the curriculum: the HIP kernels in
// ppenv_serve_curric.hip and the tests' host build (tests/csrc/serve_curric_shim.cpp, g++) compile this text and must agree BIT FOR BIT.
// Both sides are compiled with -ffp-contract=off: every product, quotient and sum below rounds on its own, the fp64 ones of the update
// included (fp64 division is correctly rounded on both).
#pragma once

#include "ppenv_serve_device.h"
#include "../../include/ppenv_serve_curric.h"

namespace pp {

// 0 when the curriculum and its cells (host memory) are acceptable; 1 .. 7 are serve_plan_invalid's rules, 8 .. 11 this header's.
PP_HD int curric_invalid(const pp_serve_curric& C, const pp_serve_cell* cells) {
    if (C.bins < 1 || C.bins > PP_CURRIC_MAX_BINS) return 8;
    if (C.num_agents != 1 && C.num_agents != 2) return 9;
    if (C.power < 0 || C.power > PP_CURRIC_MAX_POWER) return 10;
    if (!serve_finite(C.mix) || !serve_finite(C.alpha) || !(C.mix >= 0.0f && C.mix <= 1.0f) || !(C.alpha > 0.0f && C.alpha <= 1.0f)) return 11;
    pp_serve_plan P = {C.num_envs, C.env_id_offset, C.seed, C.form, C.layout, C.reset_rows, 1, C.num_envs, 0, nullptr};
    if (!cells) return serve_plan_invalid(P, nullptr);
    for (int32_t b = 0; b < C.bins; ++b)
        if (const int why = serve_plan_invalid(P, cells + b)) return why;
    return 0;
}

// The curriculum as the plan serve_draw reads: one group over all envs whose cell is cells[bin], unpaired (key = env_id_offset + e).
PP_HD pp_serve_plan curric_view(const pp_serve_curric& C, int32_t bin) {
    pp_serve_plan P = {C.num_envs, C.env_id_offset, C.seed, C.form, C.layout, C.reset_rows, 1, C.num_envs, 0, C.cells + bin};
    return P;
}

// The 24-bit integer rng_uniform(seed, gid, j, PP_CURRIC_RNG_INDEX) scales: its hash chain up to h >> 8 (ppenv_device.h).
PP_HD uint32_t curric_u24(uint64_t seed, uint32_t gid, uint32_t j) {
    uint32_t h = hash32(gid ^ (uint32_t)seed);
    h = hash32(h + j * 0x9E3779B9u + (uint32_t)(seed >> 32));
    h = hash32(h + (PP_CURRIC_RNG_INDEX + 1u) * 0x85EBCA6Bu);
    return h >> 8;
}

PP_HD uint32_t curric_uniform_cdf(int32_t B, int32_t b) { return (uint32_t)((((uint64_t)b + 1u) << 24) / (uint64_t)B); }

// #{ b in 0 .. B-2 : cdf(b) <= u24 }.  The table is non-decreasing (prefix sums of p >= 0, floored), so the count is the first index
// whose entry exceeds u24: a bisection, eight probes at most.
template <class Cdf>
PP_HD int32_t curric_bin_of(Cdf cdf, int32_t B, uint32_t u24) {
    int32_t lo = 0, hi = B - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (cdf(mid) <= u24) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct CurricTable { const uint32_t* cdf; PP_HD uint32_t operator()(int32_t b) const { return cdf[b]; } };
struct CurricUniform { int32_t B; PP_HD uint32_t operator()(int32_t b) const { return curric_uniform_cdf(B, b); } };

PP_HD int64_t curric_q(float x) {
    if (!serve_finite(x) || fabsf(x) > 2147483648.0f) return PP_CURRIC_DROPPED;
    return (int64_t)((double)x * 65536.0);
}

// serve j of env e into the buffer, drawn through `cdf`; -> its bin
template <class Cdf>
PP_HD int32_t curric_serve(const pp_serve_curric& C, int32_t B, Cdf cdf, int32_t e, uint32_t j, float* out) {
    const int32_t bin = curric_bin_of(cdf, B, curric_u24(C.seed, (uint32_t)(C.env_id_offset + e), j));
    const pp_serve_plan P = curric_view(C, bin);
    serve_store(P, e, serve_draw(P, e, j), out);
    return bin;
}

// pp_serve_curric_fill's env: drawn from the uniform table, which the fill also writes — computed here, not read, so no lane reads a word
// another workgroup writes.
PP_HD void curric_fill_env(const pp_serve_curric& C, int32_t B, int32_t e, const pp_serve_curric_state& S, float* out) {
    S.next_bin[e] = curric_serve(C, B, CurricUniform{B}, e, S.count[e], out);
    S.cur_bin[e] = -1;
    S.ret[e] = 0.0f;
}

// pp_serve_curric_step's env
PP_HD void curric_step_env(const pp_serve_curric& C, int32_t e, const float* rew, const int64_t* reset, const pp_serve_curric_state& S, float* out,
                           int32_t* fin_bin_t, int64_t* fin_q_t) {
    const float r = S.ret[e] + rew[(size_t)C.num_agents * (size_t)e];
    if (reset[(size_t)C.reset_rows * (size_t)e] == 0) {
        S.ret[e] = r;
        fin_bin_t[e] = -1;
        return;
    }
    fin_bin_t[e] = S.cur_bin[e];
    fin_q_t[e] = curric_q(r);
    S.ret[e] = 0.0f;
    S.cur_bin[e] = S.next_bin[e];
    const uint32_t j = S.count[e] + 1u;
    S.count[e] = j;
    S.next_bin[e] = curric_serve(C, C.bins, CurricTable{S.cdf}, e, j, out);
}

// What a staged entry adds to its bin's totals: -1 nothing, 0 a game (n += 1, q += fin_q), 2 a dropped game (d += 1).
PP_HD int curric_fold_kind(int32_t bin, int64_t q, int32_t B) { return bin < 0 || bin >= B ? -1 : (q == PP_CURRIC_DROPPED ? 2 : 0); }

// ---- the update, lane b per bin, in four phases with a barrier between them
// 1: the horizon's mean into the running one
PP_HD void curric_ema_bin(const pp_serve_curric& C, int32_t B, int32_t b, const int64_t* tot, int64_t* games, float* mean, int64_t* dropped) {
    const int64_t n = tot[b], q = tot[B + b], d = tot[2 * B + b];
    if (n > 0) {
        const float m = (float)((double)q / (65536.0 * (double)n));
        mean[b] = games[b] == 0 ? m : mean[b] + C.alpha * (m - mean[b]);
        games[b] += n;
    }
    dropped[b] += d;
}

// 2: the bin's weight from its rank among the seen bins
PP_HD double curric_weight_bin(const pp_serve_curric& C, int32_t B, int32_t b, const int64_t* games, const float* mean) {
    int32_t rank = 1;
    if (games[b] > 0)
        for (int32_t c = 0; c < B; ++c)
            rank += games[c] > 0 && (mean[c] < mean[b] || (mean[c] == mean[b] && c < b)) ? 1 : 0;
    const double inv = 1.0 / (double)rank;
    double w = 1.0;
    for (int32_t i = 0; i < C.power; ++i) w *= inv;
    return w;
}

// 3: its probability
PP_HD double curric_prob_bin(const pp_serve_curric& C, int32_t B, int32_t b, const double* w) {
    double W = 0.0;
    for (int32_t c = 0; c < B; ++c) W += w[c];
    return (1.0 - (double)C.mix) * w[b] / W + (double)C.mix / (double)B;
}

// 4: its entry of the table
PP_HD uint32_t curric_cdf_bin(int32_t B, int32_t b, const double* p) {
    if (b == B - 1) return 1u << 24;
    double acc = 0.0;
    for (int32_t c = 0; c <= b; ++c) acc += p[c];
    return (uint32_t)floor(16777216.0 * acc);
}

}  // namespace pp
