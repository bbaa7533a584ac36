// ppenv_ta_outcome_device.h — the arithmetic of the 27-dof task's outcome counts (include/ppenv_ta_outcome.h): one flag word into five
// sums, a window's sums into the struct, the latch rule.
//
// PP_HD like ppenv_play_device.h: the kernels that clear the count bits (ta_clear_counts_kernel in ppenv_ta.hip, the last-ticket
// workgroup of ta_chain_kernel in ppenv_ta_chain.hip), the latch kernel and the tests' host build (tests/csrc/ta_outcome_shim.cpp, g++)
// compile this text.  Integers only: the order of the additions does not matter.
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_ta_outcome.h"

namespace pp {

// c[k] += bit (16 << k) of the flag word: closer, hit_paddle, cross_net, hit_table, fall_down
PP_HD void ta_outcome_word(uint32_t f, uint32_t c[PP_TA_OUTCOME_COUNTS]) {
#pragma unroll
    for (int k = 0; k < PP_TA_OUTCOME_COUNTS; ++k) c[k] += (f >> (4 + k)) & 1u;
}

// One window (TA:1162: a step in which some env reset): the sums over all n envs, taken right before the clear, go into the running
// totals and replace the most recent window.
PP_HD void ta_outcome_window(pp_ta_outcome& o, uint64_t n, const uint32_t c[PP_TA_OUTCOME_COUNTS]) {
    o.windows += 1;
    o.envs += n;
    o.last_envs = n;
#pragma unroll
    for (int k = 0; k < PP_TA_OUTCOME_COUNTS; ++k) {
        o.count[k] += (uint64_t)c[k];
        o.last[k] = (uint64_t)c[k];
    }
}

// The latch: the copy is taken while the play totals are not frozen (play_frozen of ppenv_play_device.h: games >= games_num).
PP_HD bool ta_outcome_latches(int64_t games, int64_t games_num) { return games < games_num; }

}  // namespace pp
