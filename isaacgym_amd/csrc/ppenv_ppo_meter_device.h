// ppenv_ppo_meter_device.h — per-env and per-step arithmetic of the trainer's score meter (include/ppenv_ppo_meter.h): one env's step,
// the merge of two sets of finished games, AverageMeter.update.
//
// PP_HD like ppenv_play_device.h: the HIP kernels in ppenv_ppo_meter.hip and the tests' host build (tests/csrc/ppo_meter_shim.cpp, g++)
// compile this text.  Both sides are built with -ffp-contract=off and with signed zeros: the update's products and sums round one by
// one, so the device and the host give the same bits when they add the same terms in the same order.
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_ppo_meter.h"

namespace pp {

PP_HD void meter_clear(ppenv_ppo_meter_partial& p) {
    p.sum = 0.0;
    p.len = 0;
    p.count = 0;
    p.reserved = 0;
}

// into += from (the games of two disjoint sets of envs at the same step)
PP_HD void meter_merge(ppenv_ppo_meter_partial& into, const ppenv_ppo_meter_partial& from) {
    into.sum += from.sum;
    into.len += from.len;
    into.count += from.count;
}

// One step of one env: rl_games' `current_rewards += rewards; current_lengths += 1`, then — when agent 0's done word is non-zero — the
// finished game is left in `fin` and the running values restart at zero.  `fin` is cleared otherwise.
PP_HD void meter_env_step(float rew, int64_t done, float& cur_reward, int32_t& cur_len, ppenv_ppo_meter_partial& fin) {
    const float c = cur_reward + rew;                          // fp32, in step order
    const int32_t len = cur_len + 1;
    const bool f = done != 0;                                  // all 64 bits
    fin.sum = f ? (double)c : 0.0;
    fin.len = f ? (int64_t)len : 0;
    fin.count = f ? 1 : 0;
    fin.reserved = 0;
    cur_reward = f ? 0.0f : c;
    cur_len = f ? 0 : len;
}

// AverageMeter.update for both means with one step's finished games (p.count > 0), W = games_to_track.
PP_HD void meter_apply(ppenv_ppo_meter& m, const ppenv_ppo_meter_partial& p, int64_t w) {
    const int64_t c = (int64_t)p.count;
    const int64_t size = c < w ? c : w;
    const int64_t rest = w - size;
    const int64_t old = rest < m.current_size ? rest : m.current_size;
    const double dc = (double)c, ds = (double)size, dold = (double)old, dn = (double)(old + size);
    const double new_reward = p.sum / dc;
    const double new_length = (double)p.len / dc;
    m.mean_reward = (m.mean_reward * dold + new_reward * ds) / dn;
    m.mean_length = (m.mean_length * dold + new_length * ds) / dn;
    m.current_size = old + size;
    m.games_total += c;
    m.updates += 1;
}

}  // namespace pp
