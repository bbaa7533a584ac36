// ppo_meter_shim.cpp — the score meter's arithmetic (isaacgym_amd/csrc/ppenv_ppo_meter_device.h) compiled for the host, in the kernels'
// own summation order, as play_shim.cpp does for the play accounting.  TEST INFRASTRUCTURE ONLY.  Built by
// tests/ppo_meter_shim_binding.py with -ffp-contract=off.
#include "../../isaacgym_amd/csrc/ppenv_ppo_meter_device.h"
#include "butterfly_host.h"

namespace {

constexpr int kBlock = PPENV_PPO_METER_BLOCK;

// ppenv_ppo_meter.hip's order on an array of lanes: the xor butterfly of every wave, strides 32 down to 1, then the waves in order
ppenv_ppo_meter_partial lanes_sum(ppenv_ppo_meter_partial* lane, int n) {
    return butterfly::block_sum(lane, n, butterfly::descending,
                                [](ppenv_ppo_meter_partial& into, const ppenv_ppo_meter_partial& from) { pp::meter_merge(into, from); });
}

}  // namespace

extern "C" {

size_t ppo_meter_shim_sizeof_meter() { return sizeof(ppenv_ppo_meter); }
size_t ppo_meter_shim_sizeof_partial() { return sizeof(ppenv_ppo_meter_partial); }

// ppo_meter_update on host memory.  step_sum / step_len / step_count [h] (or NULL): S_t, L_t and c_t as the update kernel formed them.
void ppo_meter_shim_update(const float* rew, int64_t ld_rew, const int64_t* done, int64_t ld_done, int32_t h, int32_t num_envs, int32_t num_agents,
                           int64_t games_to_track, float* cur_reward, int32_t* cur_len, ppenv_ppo_meter* meter, double* step_sum,
                           int64_t* step_len, int64_t* step_count) {
    const int32_t parts = (num_envs + kBlock - 1) / kBlock;
    for (int32_t t = 0; t < h; ++t) {
        ppenv_ppo_meter_partial lanes[64];                     // meter_update_kernel's lanes: partials l, l + 64, ... in order
        for (int l = 0; l < 64; ++l) pp::meter_clear(lanes[l]);
        for (int32_t b = 0; b < parts; ++b) {                  // meter_rows_kernel's workgroup b at step t
            ppenv_ppo_meter_partial fin[kBlock];
            for (int l = 0; l < kBlock; ++l) {
                const int64_t e = (int64_t)b * kBlock + l;
                pp::meter_clear(fin[l]);
                if (e < num_envs) {
                    const size_t col = (size_t)num_agents * (size_t)e;
                    pp::meter_env_step(rew[(size_t)t * ld_rew + col], done[(size_t)t * ld_done + col], cur_reward[e], cur_len[e], fin[l]);
                }
            }
            pp::meter_merge(lanes[b % 64], lanes_sum(fin, kBlock));
        }
        const ppenv_ppo_meter_partial step = lanes_sum(lanes, 64);
        if (step_sum) step_sum[t] = step.sum;
        if (step_len) step_len[t] = step.len;
        if (step_count) step_count[t] = step.count;
        if (step.count != 0) pp::meter_apply(*meter, step, games_to_track);
    }
}

// AverageMeter.update alone: one step's (S, L, c) into the meter
void ppo_meter_shim_apply(ppenv_ppo_meter* meter, double sum, int64_t len, int32_t count, int64_t games_to_track) {
    ppenv_ppo_meter_partial p;
    p.sum = sum;
    p.len = len;
    p.count = count;
    p.reserved = 0;
    pp::meter_apply(*meter, p, games_to_track);
}

}
