// play_pair_shim.cpp — the paired-statistics arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_play_pair_device.h) compiled for
// the host, as play_shim.cpp does for the episode accounting.  TEST INFRASTRUCTURE ONLY.  Built by tests/play_pair_shim_binding.py with
// -ffp-contract=off and WITHOUT -ffinite-math-only (the table starts as NaN).
#include "../../isaacgym_amd/csrc/ppenv_play_pair_device.h"
#include "butterfly_host.h"

extern "C" {

size_t play_pair_shim_sizeof_totals() { return sizeof(pp_play_pair_totals); }

// pp_play_pair_reset on host memory
void play_pair_shim_reset(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes, float* cur_reward, int32_t* cur_steps,
                          int32_t* count, float* ret, int32_t* len) {
    const int64_t num_envs = (int64_t)envs_per_group * groups;
    for (int64_t i = 0; i < num_envs * num_agents; ++i) cur_reward[i] = 0.0f;
    for (int64_t e = 0; e < num_envs; ++e) cur_steps[e] = count[e] = 0;
    for (int64_t i = 0; i < num_envs * episodes; ++i) len[i] = 0;
    for (int64_t i = 0; i < num_envs * episodes * num_agents; ++i) ret[i] = pp::play_pair_nan();
}

// pp_play_pair_record on host memory: play_pair_record_kernel's lanes, env by env
void play_pair_shim_record(const float* rew, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes,
                           float* cur_reward, int32_t* cur_steps, int32_t* count, float* ret, int32_t* len) {
    for (int32_t e = 0; e < envs_per_group * groups; ++e) pp::play_pair_env(e, num_agents, episodes, rew, done, cur_reward, cur_steps, count, ret, len);
}

// pp_play_pair_reduce on host memory, in play_pair_reduce_kernel's order: the PPENV_PLAY_BLOCK lanes' own sums, the xor butterfly of
// every wave of 64, strides 32 down to 1, the waves in order (butterfly_host.h).
void play_pair_shim_reduce(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t episodes, const int32_t* baseline,
                           const int32_t* count, const float* ret, const int32_t* len, pp_play_pair_totals* out) {
    for (int32_t g = 0; g < groups; ++g) {
        const int32_t b = baseline[g];
        const bool ok = pp::play_pair_baseline_ok(b, groups);
        pp_play_pair_totals lane[PPENV_PLAY_BLOCK];
        for (int l = 0; l < PPENV_PLAY_BLOCK; ++l) {
            pp::play_pair_clear(lane[l]);
            if (ok) pp::play_pair_lane(l, PPENV_PLAY_BLOCK, g, b, envs_per_group, num_agents, episodes, count, ret, len, lane[l]);
        }
        pp_play_pair_totals s = butterfly::block_sum(lane, PPENV_PLAY_BLOCK, butterfly::descending,
                                                     [](pp_play_pair_totals& into, const pp_play_pair_totals& from) { pp::play_pair_merge(into, from); });
        if (!ok) s.pairs = -1;
        out[g] = s;
    }
}

}
