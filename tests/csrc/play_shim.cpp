// play_shim.cpp — the episode-accounting arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_play_device.h) compiled for the
// host, as dr_shim.cpp does for reset-time randomisation.  TEST INFRASTRUCTURE ONLY.  Built by tests/play_shim_binding.py with
// -ffp-contract=off and WITHOUT -ffinite-math-only (the minima / maxima start at +-inf).
#include "../../isaacgym_amd/csrc/ppenv_play_device.h"

extern "C" {

size_t play_shim_sizeof_totals() { return sizeof(ppenv_play_totals); }
size_t play_shim_sizeof_partial() { return sizeof(ppenv_play_partial); }

// ppenv_play_reset on host memory
void play_shim_reset(int32_t num_envs, int32_t num_agents, float* cur_reward, int32_t* cur_steps, ppenv_play_totals* totals) {
    for (int32_t i = 0; i < num_envs * num_agents; ++i) cur_reward[i] = 0.0f;
    for (int32_t e = 0; e < num_envs; ++e) cur_steps[e] = 0;
    pp::play_totals_clear(*totals);
}

// ppenv_play_accumulate on host memory: what play_rows_kernel's lanes do, env by env, one partial per PPENV_PLAY_BLOCK envs, then
// play_totals_kernel's sum of the partials — both sequential here (the device sums the same terms as a tree).
void play_shim_accumulate(const float* rew, const int64_t* done, int32_t num_envs, int32_t num_agents, int64_t games_num, float* cur_reward,
                          int32_t* cur_steps, ppenv_play_totals* totals) {
    if (pp::play_frozen(totals->games, games_num)) return;
    ppenv_play_partial launch;
    pp::play_clear(launch);
    for (int32_t b = 0; b < num_envs; b += PPENV_PLAY_BLOCK) {
        ppenv_play_partial part;
        pp::play_clear(part);
        for (int32_t e = b; e < num_envs && e < b + PPENV_PLAY_BLOCK; ++e) pp::play_env(e, num_agents, rew, done, cur_reward, cur_steps, part);
        pp::play_merge(launch, part);
    }
    pp::play_totals_add(*totals, launch);
}

}
