// ppenv_play_delay_device.h — the index rule of the control-latency delay line (include/ppenv_play_delay.h): which ring slot a row's
// sample of this control step goes to, which slot its output comes from, and the move of one 32-bit word.
//
// PP_HD like ppenv_play_act_device.h: the HIP kernel in ppenv_play_delay.hip and the tests' host build (tests/csrc/play_delay_shim.cpp,
// g++) compile this text, and the two must agree BYTE FOR BYTE.  There is no arithmetic on the values: they are moved as uint32_t words.
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_play_delay.h"

namespace pp {

// the rows a workgroup of the push kernel owns: about four words per lane, whole rows, at most one row per lane
enum { DELAY_BLOCK = 256, DELAY_WORDS = 4 * DELAY_BLOCK };

PP_HD int32_t delay_rows_per_block(int32_t width) {
    const int32_t n = DELAY_WORDS / width;
    return n < 1 ? 1 : n > DELAY_BLOCK ? DELAY_BLOCK : n;
}

// the sizes every entry accepts, and pp_play_delay_ring_bytes' arithmetic (the sanitizer build of the tests sizes its ring with it)
PP_HD bool delay_sizes_ok(int32_t rows, int32_t num_agents, int32_t width, int32_t depth) {
    return rows >= 1 && num_agents >= 1 && num_agents <= PPENV_PLAY_MAX_AGENTS && rows % num_agents == 0 && width >= 1 && width <= PP_PLAY_DELAY_MAX_WIDTH &&
           depth >= 1 && depth <= PP_PLAY_DELAY_MAX + 1;
}

PP_HD size_t delay_ring_bytes(int32_t rows, int32_t width, int32_t depth) {
    return delay_sizes_ok(rows, 1, width, depth) ? sizeof(uint32_t) * (size_t)depth * (size_t)rows * (size_t)width : 0;
}

struct delay_slots {
    int32_t write;                                               // a % K: where in[r] goes
    int32_t read;                                                // s % K: where out[r] comes from (== write: out[r] is in[r])
    int32_t next;                                                // a + 1: the row's age after this push
};

// Row r's slots for this push.  `age` is age[r] as the launch found it; done may be NULL.
PP_HD delay_slots delay_index(const int64_t* done, int32_t num_agents, int64_t r, int32_t age, int32_t d, int32_t depth) {
    const int32_t a = (done != nullptr && done[(size_t)num_agents * (size_t)(r / num_agents)] != 0) ? 0 : age;      // all 64 bits of agent 0's word
    const int32_t s = a - (a < d ? a : d);
    delay_slots o;
    o.write = (int32_t)((uint32_t)a % (uint32_t)depth);          // unsigned: an age word nobody reset still names a slot of the ring
    o.read = (int32_t)((uint32_t)s % (uint32_t)depth);
    o.next = (int32_t)((uint32_t)a + 1u);
    return o;
}

// word c of row r in slot k of the ring [K][rows][W]
PP_HD size_t delay_word(int32_t k, int64_t rows, int32_t width, int64_t r, int32_t c) {
    return ((size_t)k * (size_t)rows + (size_t)r) * (size_t)width + (size_t)c;
}

// Word c of row r: into the ring, and the delayed one out.  The slot read differs from the slot written unless the output IS the input,
// so no word is read after it was written in the same push.
PP_HD void delay_move(const uint32_t* in, int64_t ld_in, uint32_t* ring, uint32_t* out, int64_t ld_out, int64_t rows, int32_t width,
                      int64_t r, int32_t c, int32_t write, int32_t read) {
    const uint32_t v = in[(size_t)r * (size_t)ld_in + (size_t)c];
    const uint32_t o = read == write ? v : ring[delay_word(read, rows, width, r, c)];
    ring[delay_word(write, rows, width, r, c)] = v;
    out[(size_t)r * (size_t)ld_out + (size_t)c] = o;
}

}  // namespace pp
