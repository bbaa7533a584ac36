// ppenv_play_pair_device.h — per-element arithmetic of the paired episode statistics (include/ppenv_play_pair.h): one env's control
// step into the table, one lane's share of a cell's paired sums, the merge of two partial sums.
//
// PP_HD like ppenv_play_device.h: the HIP kernels in ppenv_play_pair.hip and the tests' host build (tests/csrc/play_pair_shim.cpp, g++)
// compile this text, and both must give the same bits.  The table is fp32 additions in step order and integers.  The sums are fp64:
// d = (double) a - (double) b, then d * d ROUNDED and then added — two roundings, so both builds run with -ffp-contract=off — and with
// signed zeros kept (isaacgym_amd/_lib.py SOURCE_FLAGS).  `ret` starts as quiet NaN: no -ffinite-math-only on either side.
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_play_pair.h"

namespace pp {

PP_HD float play_pair_nan() {
    const uint32_t bits = 0x7fc00000u;
    float f;
    __builtin_memcpy(&f, &bits, sizeof f);
    return f;
}

PP_HD void play_pair_clear(pp_play_pair_totals& t) {
    t.pairs = 0;
    t.steps_diff = 0;
#pragma unroll
    for (int a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) t.diff[a] = t.diff_sq[a] = t.cell[a] = t.base[a] = 0.0;
}

// into += from (two disjoint sets of pairs)
PP_HD void play_pair_merge(pp_play_pair_totals& into, const pp_play_pair_totals& from) {
    into.pairs += from.pairs;
    into.steps_diff += from.steps_diff;
#pragma unroll
    for (int a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {
        into.diff[a] += from.diff[a];
        into.diff_sq[a] += from.diff_sq[a];
        into.cell[a] += from.cell[a];
        into.base[a] += from.base[a];
    }
}

PP_HD bool play_pair_baseline_ok(int32_t b, int32_t groups) { return b >= 0 && b < groups; }

// One control step of env e: ppenv_play_device.h's running return and length; a finished game goes into row min(count[e], M) of the
// env's part of the table — when that row exists.
PP_HD void play_pair_env(int32_t e, int32_t num_agents, int32_t episodes, const float* rew, const int64_t* done, float* cur_reward,
                         int32_t* cur_steps, int32_t* count, float* ret, int32_t* len) {
    const size_t r0 = (size_t)num_agents * (size_t)e;
    const int32_t steps = cur_steps[e] + 1;
    const bool fin = done[r0] != 0;                            // all 64 bits
    const int32_t m = count[e];
    const bool keep = fin && m < episodes;
    const size_t slot = (size_t)e * (size_t)episodes + (size_t)(keep ? m : 0);
    cur_steps[e] = fin ? 0 : steps;
#pragma unroll
    for (int32_t a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {
        if (a >= num_agents) break;
        const float c = cur_reward[r0 + a] + rew[r0 + a];      // fp32, in step order
        cur_reward[r0 + a] = fin ? 0.0f : c;
        if (keep) ret[slot * (size_t)num_agents + a] = c;
    }
    if (keep) {
        len[slot] = steps;
        count[e] = m + 1;                                      // = min(m + 1, M); an env with count M is left at M
    }
}

// Lane `lane` of `block` lanes: the pairs p = lane, lane + block, ... < S * M of cell g against cell b, in order, into `acc`.
PP_HD void play_pair_lane(int32_t lane, int32_t block, int32_t g, int32_t b, int32_t envs_per_group, int32_t num_agents, int32_t episodes,
                          const int32_t* count, const float* ret, const int32_t* len, pp_play_pair_totals& acc) {
    const int64_t n = (int64_t)envs_per_group * episodes;
    const size_t eg0 = (size_t)g * (size_t)envs_per_group, eb0 = (size_t)b * (size_t)envs_per_group;
    for (int64_t p = lane; p < n; p += block) {
        const size_t i = (size_t)(p / episodes);
        const int32_t m = (int32_t)(p % episodes);
        const int32_t cg = count[eg0 + i], cb = count[eb0 + i];
        if (m >= (cg < cb ? cg : cb)) continue;
        const size_t sg = (eg0 + i) * (size_t)episodes + (size_t)m, sb = (eb0 + i) * (size_t)episodes + (size_t)m;
        acc.pairs += 1;
        acc.steps_diff += (int64_t)len[sg] - (int64_t)len[sb];
#pragma unroll
        for (int32_t a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {
            if (a >= num_agents) break;
            const double x = (double)ret[sg * (size_t)num_agents + a], y = (double)ret[sb * (size_t)num_agents + a];
            const double d = x - y;
            const double dd = d * d;
            acc.diff[a] += d;
            acc.diff_sq[a] += dd;
            acc.cell[a] += x;
            acc.base[a] += y;
        }
    }
}

}  // namespace pp
