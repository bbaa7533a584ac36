// sensor_shim.cpp — the sensor line of the HIP kernel (isaacgym_amd/csrc/ppenv_sensor_device.h) compiled for the host and walked in the
// kernel's order: workgroup by workgroup, first the rows' bookkeeping (age, episode, the level draws, the drop decision), then the column
// pairs.  TEST INFRASTRUCTURE ONLY.  Built by tests/sensor_shim_binding.py with the translation unit's own floating-point switches.
#include "../../isaacgym_amd/csrc/ppenv_sensor_device.h"

extern "C" {

int32_t sensor_shim_consts_ok(const pp_sensor_consts* c) { return pp::sensor_consts_ok(*c) ? 1 : 0; }

// U(part, key, n, k) of the header for `count` keys
void sensor_shim_uniform(uint64_t seed, int32_t channel, int32_t part, const uint32_t* key, const uint32_t* n, const uint32_t* k, int64_t count, float* out) {
    const uint64_t sd = pp::sensor_part_seed(seed, channel, part);
    for (int64_t i = 0; i < count; ++i) out[i] = pp::sensor_uniform(pp::sensor_chain(sd, key[i], n[i]), k[i]);
}

// the same through ppenv_device.h's rng_uniform: the two must be one function
void sensor_shim_rng_uniform(uint64_t seed, int32_t channel, int32_t part, const uint32_t* key, const uint32_t* n, const uint32_t* k, int64_t count, float* out) {
    const uint64_t sd = pp::sensor_part_seed(seed, channel, part);
    for (int64_t i = 0; i < count; ++i) out[i] = pp::rng_uniform(sd, key[i], n[i], k[i]);
}

void sensor_shim_box_muller(const float* u1, const float* u2, int64_t count, float* g0, float* g1) {
    for (int64_t i = 0; i < count; ++i) pp::sensor_box_muller(u1[i], u2[i], g0[i], g1[i]);
}

// pp_sensor_reset on host memory
void sensor_shim_reset(int32_t rows, int32_t* age, int32_t* episode) {
    for (int32_t r = 0; r < rows; ++r) age[r] = episode[r] = 0;
}

// pp_sensor_push on host memory; dropped [rows] (may be NULL) receives every row's drop decision
void sensor_shim_push(const uint32_t* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width, const pp_sensor_consts* consts,
                      const float* col_scale, const int32_t* col_hold, float* sigma, float* drop, int32_t* age, int32_t* episode, uint32_t* held, uint32_t* out,
                      int64_t ld_out, int32_t* dropped) {
    const pp_sensor_consts c = *consts;
    const pp::sensor_seeds sd = pp::sensor_seeds_of(c);
    const int32_t per = pp::delay_rows_per_block(width), P = (width + 1) >> 1;
    for (int64_t r0 = 0; r0 < rows; r0 += per) {                  // sensor_push_kernel, one workgroup
        const int32_t n = rows - r0 < per ? (int32_t)(rows - r0) : per;
        pp::sensor_row book[pp::DELAY_BLOCK];
        for (int32_t t = 0; t < n; ++t) {
            book[t] = pp::sensor_book(done, num_agents, r0 + t, width, c, sd, sigma, drop, age, episode);
            if (dropped) dropped[r0 + t] = book[t].dropped;
        }
        for (int32_t i = 0; i < n * P; ++i) {
            const int32_t row = i / P, p = i - row * P;
            const size_t r = (size_t)(r0 + row);
            pp::sensor_move_pair(in + r * (size_t)ld_in, held + r * (size_t)width, out + r * (size_t)ld_out, col_scale, col_hold, width, p, book[row]);
        }
    }
}

}
