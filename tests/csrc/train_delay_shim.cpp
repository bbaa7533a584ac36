// train_delay_shim.cpp — the training delay line of the HIP kernel (isaacgym_amd/csrc/ppenv_train_delay_device.h) compiled for the host and
// walked in the kernel's order: workgroup by workgroup, first the rows' bookkeeping (age, episode, the draw, delay), then the words.
// TEST INFRASTRUCTURE ONLY.  Built by tests/train_delay_shim_binding.py.
#include "../../isaacgym_amd/csrc/ppenv_train_delay_device.h"

extern "C" {

// pp::train_delay_draw for n keys: out[i] = lo + draw(seed, gid[i], episode[i], channel, hi - lo + 1)
void train_delay_shim_draws(uint64_t seed, const uint32_t* gid, const uint32_t* episode, int64_t n, int32_t channel, int32_t lo, int32_t hi, int32_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = lo + (int32_t)pp::train_delay_draw(seed, gid[i], episode[i], (uint32_t)channel, (uint32_t)(hi - lo + 1));
}

int32_t train_delay_shim_consts_ok(const pp_train_delay_consts* c) { return pp::train_delay_consts_ok(*c) ? 1 : 0; }

// pp_train_delay_reset on host memory
void train_delay_shim_reset(int32_t rows, int32_t* age, int32_t* episode) {
    for (int32_t r = 0; r < rows; ++r) age[r] = episode[r] = 0;
}

// pp_train_delay_push on host memory
void train_delay_shim_push(const uint32_t* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width,
                           const pp_train_delay_consts* consts, int32_t* delay, int32_t* age, int32_t* episode, uint32_t* ring, uint32_t* out, int64_t ld_out) {
    const pp_train_delay_consts c = *consts;
    const int32_t per = pp::delay_rows_per_block(width);
    for (int64_t r0 = 0; r0 < rows; r0 += per) {                  // train_delay_push_kernel, one workgroup
        const int32_t n = rows - r0 < per ? (int32_t)(rows - r0) : per;
        int32_t slot_write[pp::DELAY_BLOCK], slot_read[pp::DELAY_BLOCK];
        for (int32_t t = 0; t < n; ++t) {
            const pp::delay_slots s = pp::train_delay_row(done, num_agents, r0 + t, c, delay, age, episode);
            slot_write[t] = s.write;
            slot_read[t] = s.read;
        }
        for (int32_t i = 0; i < n * width; ++i) {
            const int32_t row = i / width, col = i - row * width;
            pp::delay_move(in, ld_in, ring, out, ld_out, rows, width, r0 + row, col, slot_write[row], slot_read[row]);
        }
    }
}

}
