// ppenv_dr_adr_device.h — per-env and per-slot arithmetic of automatic domain randomisation (include/ppenv_dr_adr.h has the rule).
//
// The reference has no ADR: the rule is this project's own specification, unpinned by any oracle.
//
// PP_HD like ppenv_dr_device.h, whose dr_base and dr_shape draw the interior values — the bits ppenv_dr_apply writes for a plan of the same
// ranges — and like ppenv_serve_curric_device.h, whose curric_q stages a finished game's return: the HIP kernels in ppenv_dr_adr.hip and
// the tests' host build (tests/csrc/adr_shim.cpp, g++) compile this text and must agree BIT FOR BIT.  Both sides are compiled with
// -ffp-contract=off: every product, quotient and sum below rounds on its own.
#pragma once

#include "ppenv_dr_device.h"
#include "ppenv_serve_curric_device.h"
#include "../../include/ppenv_dr_adr.h"

namespace pp {

PP_HD bool adr_finite(float x) { return serve_finite(x); }

// floor(boundary_frac * 2^24) in double; boundary_frac in [0, 1] (1 -> 1 << 24: every 24-bit coin is below it)
PP_HD uint32_t adr_thr(double boundary_frac) { return (uint32_t)floor(boundary_frac * 16777216.0); }

// 0 when the struct (host memory) and the share are acceptable; 1 .. 8 the struct's rules, 9 .. 14 a dim's (the dim in *which)
PP_HD int adr_invalid(const pp_dr_adr& A, double boundary_frac, int32_t* which) {
    *which = -1;
    if (A.num_envs < 1) return 1;
    if (A.env_id_offset < 0) return 2;
    if (A.reset_rows != 1 && A.reset_rows != 2) return 3;
    if (A.num_agents != 1 && A.num_agents != 2) return 4;
    if (A.dims < 1 || A.dims > PPENV_DR_MAX_TABLES) return 5;
    if (!(boundary_frac >= 0.0 && boundary_frac <= 1.0)) return 6;
    if (A.min_games < 1) return 7;
    if (!adr_finite(A.t_low) || !adr_finite(A.t_high) || !(A.t_low <= A.t_high)) return 8;
    for (int32_t d = 0; d < A.dims; ++d) {
        const pp_dr_adr_dim& m = A.dim[d];
        *which = d;
        if (!m.table) return 9;
        if (m.rows < 1 || m.rows > PPENV_DR_MAX_ROWS) return 10;
        if (!adr_finite(m.start_lo) || !adr_finite(m.start_hi) || !adr_finite(m.limit_lo) || !adr_finite(m.limit_hi) || !adr_finite(m.step)) return 11;
        if (!(m.step > 0.0f)) return 12;
        if (!(m.limit_lo > 0.0f)) return 13;
        if (!(m.limit_lo <= m.start_lo && m.start_lo <= m.start_hi && m.start_hi <= m.limit_hi)) return 14;
    }
    *which = -1;
    return 0;
}

// The 24-bit integer rng_uniform(sd, gid, j, k) scales: its hash chain up to h >> 8 (ppenv_device.h), as curric_u24 obtains its one.
PP_HD uint32_t adr_u24(uint64_t sd, uint32_t gid, uint32_t j, uint32_t k) {
    uint32_t h = hash32(gid ^ (uint32_t)sd);
    h = hash32(h + j * 0x9E3779B9u + (uint32_t)(sd >> 32));
    h = hash32(h + (k + 1u) * 0x85EBCA6Bu);
    return h >> 8;
}

// The slot of redraw j of global env gid: a boundary 0 .. 2 D - 1 for a boundary worker, 2 D (interior) otherwise.
PP_HD int32_t adr_slot_of(uint64_t seed, uint32_t gid, uint32_t j, uint32_t thr, int32_t D) {
    const uint64_t sd = seed ^ PPENV_DR_SEED_SALT;
    if (!(adr_u24(sd, gid, j, PP_ADR_COIN_INDEX) < thr)) return 2 * D;
    return (int32_t)(((uint64_t)adr_u24(sd, gid, j, PP_ADR_PICK_INDEX) * (uint64_t)(2 * D)) >> 24);
}

// Where DRAW takes its ranges from: the state's range[] (the step), or the struct's starts (the fill, which also WRITES range[] — the
// starts are computed here, not read, so no lane reads a word another workgroup writes).
struct AdrRanges { const float* range; PP_HD float operator()(const pp_dr_adr&, int32_t d, int32_t s) const { return range[2 * d + s]; } };
struct AdrStarts { PP_HD float operator()(const pp_dr_adr& A, int32_t d, int32_t s) const { return s ? A.dim[d].start_hi : A.dim[d].start_lo; } };

// DRAW(e, j): column e of every dim's table, -> the slot.  Consecutive lanes = consecutive envs of one row: each store is coalesced.
template <class Range>
PP_HD int32_t adr_draw(const pp_dr_adr& A, int32_t D, Range range, int32_t e, uint32_t j) {
    const uint32_t gid = (uint32_t)(A.env_id_offset + e);
    const int32_t slot = adr_slot_of(A.seed, gid, j, A.thr, D);
    for (int32_t d = 0; d < D; ++d) {
        const pp_dr_adr_dim& m = A.dim[d];
        const float lo = range(A, d, 0), hi = range(A, d, 1);
        const bool pinned = slot < 2 * D && (slot >> 1) == d;
        const float pin = (slot & 1) ? hi : lo;
        for (int32_t r = 0; r < m.rows; ++r)
            m.table[(size_t)r * (size_t)A.num_envs + (size_t)e] =
                pinned ? pin : dr_shape(dr_base(A.seed, gid, j, dr_key(d, r), PPENV_DR_UNIFORM), PPENV_DR_UNIFORM, PPENV_DR_SCALING, lo, hi, 1.0f);
    }
    return slot;
}

// pp_dr_adr_fill's env
PP_HD void adr_fill_env(const pp_dr_adr& A, int32_t D, int32_t e, const pp_dr_adr_state& S) {
    const int32_t j = S.draws[e];
    S.draws[e] = j + 1;
    (void)adr_draw(A, D, AdrStarts{}, e, (uint32_t)j);
    S.slot[e] = -1;
    S.ret[e] = 0.0f;
}

// pp_dr_adr_step's env.  The caller has bounded e by the size the state was made for; the struct's num_envs bounds the table columns.
// ret[e] and the struct's scalars leave together, rew and reset follow: an idle lane waits for two memory round trips.
PP_HD void adr_step_env(const pp_dr_adr& A, int32_t e, const float* rew, const int64_t* reset, const pp_dr_adr_state& S, int32_t* fin_slot_t,
                        int64_t* fin_q_t) {
    const float r0 = S.ret[e];
    const int32_t agents = A.num_agents, rows = A.reset_rows;
    const float r = r0 + rew[(size_t)agents * (size_t)e];
    if (reset[(size_t)rows * (size_t)e] == 0) {
        S.ret[e] = r;
        fin_slot_t[e] = -1;
        return;
    }
    fin_slot_t[e] = S.slot[e];
    fin_q_t[e] = curric_q(r);
    S.ret[e] = 0.0f;
    if (e >= A.num_envs) return;
    const int32_t j = S.draws[e];
    S.draws[e] = j + 1;
    S.slot[e] = adr_draw(A, A.dims, AdrRanges{S.range}, e, (uint32_t)j);
}

// pp_dr_adr_update's slot s of S = 2 D + 1: every word it writes (its own per-slot state, and range[s] for a boundary slot) is its alone.
PP_HD void adr_update_slot(const pp_dr_adr& A, int32_t D, int32_t s, const int64_t* tot, const pp_dr_adr_state& S) {
    const int32_t slots = 2 * D + 1;
    const int64_t n = tot[s], q = tot[slots + s], d = tot[2 * slots + s];
    S.games[s] += n;
    S.dropped[s] += d;
    int64_t an = S.acc_n[s] + n, aq = S.acc_q[s] + q;
    if (an >= (int64_t)A.min_games) {
        const float m = (float)((double)aq / (65536.0 * (double)an));
        S.mean[s] = m;
        if (s < 2 * D) {
            const pp_dr_adr_dim& dim = A.dim[s >> 1];
            const float v = S.range[s];                                  // range[d][side] is word 2 d + side
            if (m >= A.t_high) {
                S.range[s] = (s & 1) ? fminf(v + dim.step, dim.limit_hi) : fmaxf(v - dim.step, dim.limit_lo);
                S.widened[s] += 1;
            } else if (m <= A.t_low) {
                S.range[s] = (s & 1) ? fmaxf(v - dim.step, dim.start_hi) : fminf(v + dim.step, dim.start_lo);
                S.narrowed[s] += 1;
            }
        }
        an = aq = 0;
    }
    S.acc_n[s] = an;
    S.acc_q[s] = aq;
}

}  // namespace pp
