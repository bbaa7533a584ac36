// ppenv_play_device.h — per-env arithmetic of episode accounting (include/ppenv_play.h): one env's control step, the merge of two
// sets of finished games, the totals' update.
//
// PP_HD like ppenv_dr_device.h: the HIP kernels in ppenv_play.hip and the tests' host build (tests/csrc/play_shim.cpp, g++) compile
// this text.  What must agree bit for bit between the two — and with rl_games' loop — is the integer state and cur_reward: one fp32
// addition per row and step, nothing that could fuse.  The fp64 sums are plain additions of exactly representable terms (a float, the
// exact square of a float); only their ORDER differs between the device's tree and a sequential host loop.
// The minima / maxima start at +-inf: this header is compiled without -ffinite-math-only on both sides (isaacgym_amd/_lib.py
// SOURCE_FLAGS).
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_play.h"

namespace pp {

PP_HD float play_inf() { return __builtin_huge_valf(); }

PP_HD void play_clear(ppenv_play_partial& p) {
    p.games = 0;
    p.steps = 0;
#pragma unroll
    for (int a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {
        p.reward[a] = 0.0;
        p.reward_sq[a] = 0.0;
        p.reward_min[a] = play_inf();
        p.reward_max[a] = -play_inf();
    }
}

// into += from (the games of two disjoint sets of envs)
PP_HD void play_merge(ppenv_play_partial& into, const ppenv_play_partial& from) {
    into.games += from.games;
    into.steps += from.steps;
#pragma unroll
    for (int a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {
        into.reward[a] += from.reward[a];
        into.reward_sq[a] += from.reward_sq[a];
        into.reward_min[a] = from.reward_min[a] < into.reward_min[a] ? from.reward_min[a] : into.reward_min[a];
        into.reward_max[a] = from.reward_max[a] > into.reward_max[a] ? from.reward_max[a] : into.reward_max[a];
    }
}

// The freeze: the launch changes nothing once games_num games are counted.
PP_HD bool play_frozen(int64_t games, int64_t games_num) { return games >= games_num; }

// One control step of env e: rl_games' `cr += r; steps += 1`, then — when agent 0's done word is non-zero — the finished game goes
// into `acc` and the env's running values are zeroed.  `acc` is the caller's own (a lane's, or a host loop's).
PP_HD void play_env(int32_t e, int32_t num_agents, const float* rew, const int64_t* done, float* cur_reward, int32_t* cur_steps,
                    ppenv_play_partial& acc) {
    const size_t r0 = (size_t)num_agents * (size_t)e;
    const int32_t len = cur_steps[e] + 1;
    const bool fin = done[r0] != 0;                            // all 64 bits
    cur_steps[e] = fin ? 0 : len;
#pragma unroll
    for (int32_t a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {      // a constant trip count: `acc` is indexed by constants only
        if (a >= num_agents) break;
        const float c = cur_reward[r0 + a] + rew[r0 + a];      // fp32, in step order
        cur_reward[r0 + a] = fin ? 0.0f : c;
        if (fin) {
            const double d = (double)c;
            acc.reward[a] += d;
            acc.reward_sq[a] += d * d;                         // d * d is exact in fp64 (24-bit significand squared)
            acc.reward_min[a] = c < acc.reward_min[a] ? c : acc.reward_min[a];
            acc.reward_max[a] = c > acc.reward_max[a] ? c : acc.reward_max[a];
        }
    }
    if (fin) {
        acc.games += 1;
        acc.steps += (int64_t)len;
    }
}

// totals += the launch's games; one more control step counted
PP_HD void play_totals_add(ppenv_play_totals& t, const ppenv_play_partial& p) {
    t.games += p.games;
    t.steps += p.steps;
    t.launches += 1;
#pragma unroll
    for (int a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {
        t.reward[a] += p.reward[a];
        t.reward_sq[a] += p.reward_sq[a];
        t.reward_min[a] = p.reward_min[a] < t.reward_min[a] ? p.reward_min[a] : t.reward_min[a];
        t.reward_max[a] = p.reward_max[a] > t.reward_max[a] ? p.reward_max[a] : t.reward_max[a];
    }
}

PP_HD void play_totals_clear(ppenv_play_totals& t) {
    t.games = 0;
    t.steps = 0;
    t.launches = 0;
#pragma unroll
    for (int a = 0; a < PPENV_PLAY_MAX_AGENTS; ++a) {
        t.reward[a] = 0.0;
        t.reward_sq[a] = 0.0;
        t.reward_min[a] = play_inf();
        t.reward_max[a] = -play_inf();
    }
}

}  // namespace pp
