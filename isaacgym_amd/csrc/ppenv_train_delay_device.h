// ppenv_train_delay_device.h — what the training delay line (include/ppenv_train_delay.h) adds to play's: the integer draw of a row's delay
// and the row's bookkeeping for one push (age, episode, delay -> the two ring slots).  The index rule and the move of a word are
// ppenv_play_delay_device.h's, by inclusion.
//
// PP_HD: the HIP kernel in ppenv_train_delay.hip and the tests' host build (tests/csrc/train_delay_shim.cpp, g++) compile this text, and the
// two must agree BYTE FOR BYTE.  There is no floating point here.
#pragma once

#include "ppenv_play_delay_device.h"
#include "../../include/ppenv_train_delay.h"

namespace pp {

PP_HD bool train_delay_consts_ok(const pp_train_delay_consts& c) {
    return c.lo >= 0 && c.lo <= c.hi && c.hi <= PP_PLAY_DELAY_MAX && (c.channel == PP_TRAIN_DELAY_COMMAND || c.channel == PP_TRAIN_DELAY_SENSING);
}

// rng_uniform's hash chain (ppenv_device.h), keyed (seed, gid, episode = n, k), reduced to 0 .. span - 1 in integers: the 24 bits
// rng_uniform would turn into a float, times span, shifted down.  span <= 16: the product has at most 28 bits.  span == 1 -> 0.
PP_HD uint32_t train_delay_draw(uint64_t seed, uint32_t gid, uint32_t n, uint32_t k, uint32_t span) {
    uint32_t h = hash32(gid ^ (uint32_t)seed);
    h = hash32(h + n * 0x9E3779B9u + (uint32_t)(seed >> 32));
    h = hash32(h + (k + 1u) * 0x85EBCA6Bu);
    return (uint32_t)(((uint64_t)(h >> 8) * span) >> 24);
}

// Row r's push: the only read and the only write of age[r]; where this sample is the first of an episode, episode[r] is counted up and
// delay[r] redrawn.  -> the row's slots.  delay_index is asked ONCE, with the delay the row holds: its `next` says whether this sample is
// the first of an episode (a == 0 <=> next == 1), and at a == 0 the slots are (0, 0) whatever delay >= 0 went in (s = a - min(a, d) = 0),
// so the redrawn delay needs no second call — which the compiler does not fold into the first: it would repeat delay_index's 64-bit
// division and its read of `done` behind the first's.  A negative held word (a table nobody initialised) counts as 0 for that reason.
// The row's three words are read up front and the draw is formed for every row, first or not: read only where an episode starts,
// episode[r] would be a second trip to memory behind age[r] and done, on the one lane per row the workgroup's barrier waits for
// (DESIGN §6 "Training under latency").  Only the two stores are conditional.
PP_HD delay_slots train_delay_row(const int64_t* done, int32_t num_agents, int64_t r, const pp_train_delay_consts& c, int32_t* delay, int32_t* age,
                                  int32_t* episode) {
    const int32_t age_r = age[r], word = delay[r], held = word < 0 ? 0 : word;
    const uint32_t n = (uint32_t)episode[r];
    const uint32_t env = (uint32_t)r / (uint32_t)num_agents;     // r < rows <= 2^31 - 1: a 32-bit division, not the 64-bit one r / num_agents would be
    const int32_t drawn = c.lo + (int32_t)train_delay_draw(c.seed, (uint32_t)c.env_id_offset + env, n, (uint32_t)c.channel, (uint32_t)(c.hi - c.lo + 1));
    const delay_slots s = delay_index(done, num_agents, r, age_r, held, c.hi + 1);
    if (s.next == 1) {                                           // the first sample of an episode: slots (0, 0)
        episode[r] = (int32_t)(n + 1u);
        delay[r] = drawn;
    }
    age[r] = s.next;
    return s;
}

}  // namespace pp
