// ppo_meter_shim.cpp — the score meter's arithmetic (isaacgym_amd/csrc/ppenv_ppo_meter_device.h) compiled for the host, in the kernels'
// own summation order, as play_shim.cpp does for the play accounting.  TEST INFRASTRUCTURE ONLY.  Built by
// tests/ppo_meter_shim_binding.py with -ffp-contract=off.
#include "../../isaacgym_amd/csrc/ppenv_ppo_meter_device.h"

namespace {

constexpr int kBlock = PPENV_PPO_METER_BLOCK;

// wave_merge of ppenv_ppo_meter.hip on 64 lanes' values: the xor butterfly, stage by stage; every lane ends with lane 0's bits.
void butterfly(ppenv_ppo_meter_partial* v) {
    for (int off = 32; off >= 1; off >>= 1) {
        ppenv_ppo_meter_partial next[64];
        for (int i = 0; i < 64; ++i) {
            next[i] = v[i];
            pp::meter_merge(next[i], v[i ^ off]);
        }
        for (int i = 0; i < 64; ++i) v[i] = next[i];
    }
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
            ppenv_ppo_meter_partial part;
            for (int w = 0; w < kBlock / 64; ++w) {
                ppenv_ppo_meter_partial fin[64];
                for (int l = 0; l < 64; ++l) {
                    const int64_t e = (int64_t)b * kBlock + w * 64 + l;
                    pp::meter_clear(fin[l]);
                    if (e < num_envs) {
                        const size_t col = (size_t)num_agents * (size_t)e;
                        pp::meter_env_step(rew[(size_t)t * ld_rew + col], done[(size_t)t * ld_done + col], cur_reward[e], cur_len[e], fin[l]);
                    }
                }
                butterfly(fin);
                if (w == 0) part = fin[0];
                else pp::meter_merge(part, fin[0]);
            }
            pp::meter_merge(lanes[b % 64], part);
        }
        butterfly(lanes);
        if (step_sum) step_sum[t] = lanes[0].sum;
        if (step_len) step_len[t] = lanes[0].len;
        if (step_count) step_count[t] = lanes[0].count;
        if (lanes[0].count != 0) pp::meter_apply(*meter, lanes[0], games_to_track);
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
