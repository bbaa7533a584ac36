// ppenv_sensor.hip — the sensor line on the device (include/ppenv_sensor.h): additive Gaussian noise with a per-row amplitude and a per-column
// scale, and per-row sample dropouts that hold the values last delivered.
//
//   sensor_push_kernel   the delay lines' shape: workgroup b owns the rows [b * R, b * R + R), R = pp::delay_rows_per_block(W) (the ragged last
//                        workgroup guarded).  Lane t < R does row t's bookkeeping (pp::sensor_book: the only read and write of the row's age
//                        and episode, at a drawn episode start of its sigma and drop, and the drop decision) and leaves the row's noise chain,
//                        draw base, amplitude and drop flag in LDS; after the barrier the 256 lanes walk the workgroup's R * P column pairs
//                        in order (P = (W + 1) / 2), consecutive lanes on consecutive pairs (pp::sensor_move_pair).
//   sensor_reset_kernel  age and episode to zero (grid-stride).
// No atomics, no counter on the host: a push is a function of the device words and the by-value constants alone, so a captured launch
// replays like an eager one.  A workgroup writes age, episode, sigma, drop, held and out of its own rows only, and reads nothing another
// writes.  Plain C++ stores.
//
// Memory: 2 * rows * W words (in, out) plus one word per hold column (held: written, or read where the sample is dropped), col_scale and
// col_hold once per workgroup from L2, and per row four words of bookkeeping.  Arithmetic: per noised pair two hash rounds and one Box-Muller
// on the hardware's transcendentals; a pair whose two scales are zero draws nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_sensor_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = pp::DELAY_BLOCK;
constexpr int kResetBlocks = 1024;                              // the reset's grid-stride cap

__global__ __launch_bounds__(kBlock) void sensor_push_kernel(const uint32_t* __restrict__ in, int64_t ld_in, const int64_t* __restrict__ done, int32_t rows,
                                                             int32_t num_agents, int32_t width, int32_t rows_per_block, pp_sensor_consts c, pp::sensor_seeds sd,
                                                             const float* __restrict__ col_scale, const int32_t* __restrict__ col_hold,
                                                             float* __restrict__ sigma, float* __restrict__ drop, int32_t* __restrict__ age,
                                                             int32_t* __restrict__ episode, uint32_t* __restrict__ held, uint32_t* __restrict__ out, int64_t ld_out) {
    __shared__ pp::sensor_row book[kBlock];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;     // < rows: the grid is ceil(rows / rows_per_block)
    const int32_t left = (int32_t)((int64_t)rows - r0);
    const int32_t n = left < rows_per_block ? left : rows_per_block;      // 1 .. kBlock rows
    if (tid < n) book[tid] = pp::sensor_book(done, num_agents, r0 + tid, width, c, sd, sigma, drop, age, episode);
    __syncthreads();
    const int32_t P = (width + 1) >> 1;
    const int32_t pairs = n * P;                                 // <= max(1024 / 2 + 256, 256)
    for (int32_t i = tid; i < pairs; i += kBlock) {
        const int32_t row = i / P, p = i - row * P;
        const size_t r = (size_t)(r0 + row);
        pp::sensor_move_pair(in + r * (size_t)ld_in, held + r * (size_t)width, out + r * (size_t)ld_out, col_scale, col_hold, width, p, book[row]);
    }
}

__global__ __launch_bounds__(kBlock) void sensor_reset_kernel(int32_t rows, int32_t* __restrict__ age, int32_t* __restrict__ episode) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        age[i] = 0;
        episode[i] = 0;
    }
}

}  // namespace

extern "C" size_t pp_sensor_table_bytes(int32_t rows) {
    return rows >= 1 ? sizeof(int32_t) * (size_t)rows : 0;
}

extern "C" size_t pp_sensor_held_bytes(int32_t rows, int32_t width) {
    return pp::sensor_held_bytes(rows, width);
}

extern "C" int pp_sensor_reset(int32_t rows, int32_t* age, int32_t* episode, void* stream) {
    if (rows < 1 || !age || !episode) {
        pp_set_errorf("pp_sensor_reset: NULL pointer or rows < 1");
        return PPENV_EINVAL;
    }
    const int64_t blocks = ((int64_t)rows + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(sensor_reset_kernel, dim3((uint32_t)(blocks < kResetBlocks ? blocks : kResetBlocks)), dim3(kBlock), 0, (hipStream_t)stream, rows, age, episode);
    return pp_launched("launching sensor_reset_kernel failed");
}

extern "C" int pp_sensor_push(const float* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width,
                              const pp_sensor_consts* consts, const float* col_scale, const int32_t* col_hold, float* sigma, float* drop, int32_t* age,
                              int32_t* episode, float* held, float* out, int64_t ld_out, void* stream) {
    if (!consts) {
        pp_set_errorf("pp_sensor_push: NULL constants");
        return PPENV_EINVAL;
    }
    const pp_sensor_consts c = *consts;
    if (!pp::sensor_range_ok(c.sigma_lo, c.sigma_hi, 3.4028234664e38f)) {
        pp_set_errorf("pp_sensor_push: sigma_lo %g, sigma_hi %g: need finite 0 <= lo <= hi", (double)c.sigma_lo, (double)c.sigma_hi);
        return PPENV_EINVAL;
    }
    if (!pp::sensor_range_ok(c.drop_lo, c.drop_hi, 1.0f)) {
        pp_set_errorf("pp_sensor_push: drop_lo %g, drop_hi %g: need 0 <= lo <= hi <= 1", (double)c.drop_lo, (double)c.drop_hi);
        return PPENV_EINVAL;
    }
    if (c.draw != 0 && c.draw != 1) {
        pp_set_errorf("pp_sensor_push: draw %d is not 0 (the caller's table) or 1 (drawn per episode)", c.draw);
        return PPENV_EINVAL;
    }
    if (c.key_period < 0 || c.env_id_offset < 0) {
        pp_set_errorf("pp_sensor_push: key_period %d or env_id_offset %d < 0", c.key_period, c.env_id_offset);
        return PPENV_EINVAL;
    }
    if (c.channel != PP_SENSOR_COMMAND && c.channel != PP_SENSOR_SENSING) {
        pp_set_errorf("pp_sensor_push: channel %d is not 0 (command) or 1 (sensing)", c.channel);
        return PPENV_EINVAL;
    }
    if (!pp::delay_sizes_ok(rows, num_agents, width, 1) || !in || !col_scale || !col_hold || !sigma || !drop || !age || !episode || !held || !out || ld_in < width ||
        ld_out < width) {
        pp_set_errorf("pp_sensor_push: NULL pointer (done excepted), rows < 1 or no multiple of num_agents, num_agents not 1 or 2, width outside 1..%d, "
                      "or a stride below width", PP_PLAY_DELAY_MAX_WIDTH);
        return PPENV_EINVAL;
    }
    const int32_t per = pp::delay_rows_per_block(width);
    const int64_t blocks = ((int64_t)rows + per - 1) / per;      // <= rows <= 2^31 - 1
    hipLaunchKernelGGL(sensor_push_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t*)in, ld_in, done, rows, num_agents, width,
                       per, c, pp::sensor_seeds_of(c), col_scale, col_hold, sigma, drop, age, episode, (uint32_t*)held, (uint32_t*)out, ld_out);
    return pp_launched("launching sensor_push_kernel failed");
}
