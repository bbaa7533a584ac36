// play_delay_shim.cpp — the control-latency delay line of the HIP kernel (isaacgym_amd/csrc/ppenv_play_delay_device.h) compiled for the
// host and walked in the kernel's order: workgroup by workgroup, first the rows' slots and ages, then the words.  TEST INFRASTRUCTURE
// ONLY.  Built by tests/play_delay_shim_binding.py.
#include "../../isaacgym_amd/csrc/ppenv_play_delay_device.h"

extern "C" {

int32_t play_delay_shim_rows_per_block(int32_t width) { return pp::delay_rows_per_block(width); }

// pp_play_delay_reset on host memory
void play_delay_shim_reset(int32_t rows, int32_t* age) {
    for (int32_t r = 0; r < rows; ++r) age[r] = 0;
}

// pp_play_delay_push on host memory
void play_delay_shim_push(const uint32_t* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width, int32_t depth,
                          const int32_t* delay, int32_t* age, uint32_t* ring, uint32_t* out, int64_t ld_out) {
    const int32_t per = pp::delay_rows_per_block(width);
    for (int64_t r0 = 0; r0 < rows; r0 += per) {                  // play_delay_push_kernel, one workgroup
        const int32_t n = rows - r0 < per ? (int32_t)(rows - r0) : per;
        int32_t slot_write[pp::DELAY_BLOCK], slot_read[pp::DELAY_BLOCK];
        for (int32_t t = 0; t < n; ++t) {
            const pp::delay_slots s = pp::delay_index(done, num_agents, r0 + t, age[r0 + t], delay[r0 + t], depth);
            slot_write[t] = s.write;
            slot_read[t] = s.read;
            age[r0 + t] = s.next;
        }
        for (int32_t i = 0; i < n * width; ++i) {
            const int32_t row = i / width, c = i - row * width;
            pp::delay_move(in, ld_in, ring, out, ld_out, rows, width, r0 + row, c, slot_write[row], slot_read[row]);
        }
    }
}

}
