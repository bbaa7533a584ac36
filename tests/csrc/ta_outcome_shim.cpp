// ta_outcome_shim.cpp — the outcome-count arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_ta_outcome_device.h) compiled for the
// host, as play_shim.cpp does for the episode accounting.  TEST INFRASTRUCTURE ONLY.  Built by tests/ta_outcome_shim_binding.py.
#include "../../isaacgym_amd/csrc/ppenv_ta_outcome_device.h"

extern "C" {

size_t ta_outcome_shim_sizeof() { return sizeof(pp_ta_outcome); }
// byte offsets of windows, envs, count, last_envs, last, reserved
void ta_outcome_shim_offsets(size_t out[6]) {
    out[0] = offsetof(pp_ta_outcome, windows); out[1] = offsetof(pp_ta_outcome, envs); out[2] = offsetof(pp_ta_outcome, count);
    out[3] = offsetof(pp_ta_outcome, last_envs); out[4] = offsetof(pp_ta_outcome, last); out[5] = offsetof(pp_ta_outcome, reserved);
}

// ta_clear_counts_kernel on host memory: when `any`, the five count bits of all n flag words are summed into *outcome (NULL: off)
// and then cleared — sequentially here (the device sums the same integers as a tree).
void ta_outcome_shim_clear(int32_t n, uint32_t* flags, int32_t any, pp_ta_outcome* outcome) {
    if (!any) return;
    uint32_t c[PP_TA_OUTCOME_COUNTS] = {0u, 0u, 0u, 0u, 0u};
    for (int32_t i = 0; i < n; ++i) {
        pp::ta_outcome_word(flags[i], c);
        flags[i] &= ~PPENV_TA_COUNT_MASK;
    }
    if (outcome) pp::ta_outcome_window(*outcome, (uint64_t)n, c);
}

// ta_outcome_latch_kernel on host memory
void ta_outcome_shim_latch(const pp_ta_outcome* live, int64_t games, int64_t games_num, pp_ta_outcome* latched) {
    if (pp::ta_outcome_latches(games, games_num)) *latched = *live;
}

}
