// ppenv_train_delay.hip — the control-latency delay line of training, on the device (include/ppenv_train_delay.h): play's per-row ring
// (ppenv_play_delay.hip) whose delay is redrawn by the kernel at every episode start.
//
//   train_delay_push_kernel   play_delay_push_kernel's shape: workgroup b owns the rows [b * R, b * R + R), R = pp::delay_rows_per_block(W)
//                             (the ragged last workgroup guarded).  Lane t < R does row t's bookkeeping (pp::train_delay_row: the only read
//                             and write of the row's age, and at an episode start of its episode count and delay, with one hash chain) and
//                             leaves the two slots in LDS; after the barrier the 256 lanes walk the workgroup's R * W words in order.
//   train_delay_reset_kernel  age and episode to zero (grid-stride).
// No atomics, no counter on the host: a push is a function of the device words and the by-value constants alone, so a captured launch
// replays like an eager one.  A workgroup writes age, episode, delay, ring and out of its own rows only, and reads nothing another writes.
//
// Memory: play's 3 * rows * W words (2 where the delay is 0), plus per row the delay word (read, or written at an episode start) and at an
// episode start the episode word (read and written).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_train_delay_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = pp::DELAY_BLOCK;
constexpr int kResetBlocks = 1024;                              // the reset's grid-stride cap

__global__ __launch_bounds__(kBlock) void train_delay_push_kernel(const uint32_t* __restrict__ in, int64_t ld_in, const int64_t* __restrict__ done, int32_t rows,
                                                                  int32_t num_agents, int32_t width, int32_t rows_per_block, pp_train_delay_consts c,
                                                                  int32_t* __restrict__ delay, int32_t* __restrict__ age, int32_t* __restrict__ episode,
                                                                  uint32_t* ring, uint32_t* __restrict__ out, int64_t ld_out) {
    __shared__ int32_t slot_write[kBlock], slot_read[kBlock];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;     // < rows: the grid is ceil(rows / rows_per_block)
    const int32_t left = (int32_t)((int64_t)rows - r0);
    const int32_t n = left < rows_per_block ? left : rows_per_block;      // 1 .. kBlock rows
    if (tid < n) {
        const pp::delay_slots s = pp::train_delay_row(done, num_agents, r0 + tid, c, delay, age, episode);
        slot_write[tid] = s.write;
        slot_read[tid] = s.read;
    }
    __syncthreads();
    const int32_t words = n * width;                             // <= max(1024, 512)
    for (int32_t i = tid; i < words; i += kBlock) {
        const int32_t row = i / width, col = i - row * width;
        pp::delay_move(in, ld_in, ring, out, ld_out, rows, width, r0 + row, col, slot_write[row], slot_read[row]);
    }
}

__global__ __launch_bounds__(kBlock) void train_delay_reset_kernel(int32_t rows, int32_t* __restrict__ age, int32_t* __restrict__ episode) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        age[i] = 0;
        episode[i] = 0;
    }
}

}  // namespace

extern "C" size_t pp_train_delay_ring_bytes(int32_t rows, int32_t width, int32_t hi) {
    return hi >= 0 && hi <= PP_PLAY_DELAY_MAX ? pp::delay_ring_bytes(rows, width, hi + 1) : 0;
}

extern "C" size_t pp_train_delay_table_bytes(int32_t rows) {
    return rows >= 1 ? sizeof(int32_t) * (size_t)rows : 0;
}

extern "C" int pp_train_delay_reset(int32_t rows, int32_t* age, int32_t* episode, void* stream) {
    if (rows < 1 || !age || !episode) {
        pp_set_errorf("pp_train_delay_reset: NULL pointer or rows < 1");
        return PPENV_EINVAL;
    }
    const int64_t blocks = ((int64_t)rows + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(train_delay_reset_kernel, dim3((uint32_t)(blocks < kResetBlocks ? blocks : kResetBlocks)), dim3(kBlock), 0, (hipStream_t)stream, rows, age,
                       episode);
    return pp_launched("launching train_delay_reset_kernel failed");
}

extern "C" int pp_train_delay_push(const float* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width,
                                   const pp_train_delay_consts* consts, int32_t* delay, int32_t* age, int32_t* episode, float* ring, float* out,
                                   int64_t ld_out, void* stream) {
    if (!consts) {
        pp_set_errorf("pp_train_delay_push: NULL constants");
        return PPENV_EINVAL;
    }
    const pp_train_delay_consts c = *consts;
    if (c.lo < 0) {
        pp_set_errorf("pp_train_delay_push: lo %d < 0", c.lo);
        return PPENV_EINVAL;
    }
    if (c.lo > c.hi) {
        pp_set_errorf("pp_train_delay_push: lo %d > hi %d", c.lo, c.hi);
        return PPENV_EINVAL;
    }
    if (c.hi > PP_PLAY_DELAY_MAX) {
        pp_set_errorf("pp_train_delay_push: hi %d > %d", c.hi, PP_PLAY_DELAY_MAX);
        return PPENV_EINVAL;
    }
    if (c.channel != PP_TRAIN_DELAY_COMMAND && c.channel != PP_TRAIN_DELAY_SENSING) {
        pp_set_errorf("pp_train_delay_push: channel %d is not 0 (command) or 1 (sensing)", c.channel);
        return PPENV_EINVAL;
    }
    if (!pp::delay_sizes_ok(rows, num_agents, width, c.hi + 1) || !in || !delay || !age || !episode || !ring || !out || ld_in < width || ld_out < width) {
        pp_set_errorf("pp_train_delay_push: NULL pointer (done excepted), rows < 1 or no multiple of num_agents, num_agents not 1 or 2, width outside 1..%d, "
                      "or a stride below width", PP_PLAY_DELAY_MAX_WIDTH);
        return PPENV_EINVAL;
    }
    const int32_t per = pp::delay_rows_per_block(width);
    const int64_t blocks = ((int64_t)rows + per - 1) / per;      // <= rows <= 2^31 - 1
    hipLaunchKernelGGL(train_delay_push_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t*)in, ld_in, done, rows, num_agents,
                       width, per, c, delay, age, episode, (uint32_t*)ring, (uint32_t*)out, ld_out);
    return pp_launched("launching train_delay_push_kernel failed");
}
