// ppenv_play_delay.hip — the control-latency delay line of a played checkpoint, on the device (include/ppenv_play_delay.h): per row a
// ring of the last K samples of a [rows, W] tensor; a push stores this control step's sample and hands out the one d[r] steps old.
//
//   play_delay_push_kernel   workgroup b owns the rows [b * R, b * R + R), R = pp::delay_rows_per_block(W) whole rows of about 1024 words in
//                            all (the ragged last workgroup guarded): lane t < R reads age of row t — the only read of that word in the
//                            launch — and done and d[r], leaves the row's two slots in LDS and writes the age; after the barrier the 256
//                            lanes walk the workgroup's R * W words in order, consecutive lanes on consecutive words of a row.
//   play_delay_reset_kernel  age to zero (grid-stride).
// No atomics, no counter on the host: what a push does is a function of the device words alone, so a captured launch replays like an
// eager one.  A workgroup writes age, ring and out of its own rows only, and reads nothing another workgroup writes.
//
// Memory.  A push moves 3 * rows * W words (in -> ring, ring -> out; 2 where the delay is 0).  Rows are contiguous in `in` / `out` up to
// their stride and in a slot of the ring, and neighbouring rows mostly share a slot (they restart at different times only after their
// first reset), so a wave's 64 lanes touch one to a few runs of contiguous 4-byte words whatever W is: 27, 313 and a stride of W + 1
// cost nothing extra.  Wider accesses would need W, both strides and the base addresses to be multiples of 4 words, which the callers'
// shapes (7, 27, 80, 313; the [rows, A + 1] head buffer) are not; at the sizes played (0.2 .. 5 MB a push) the launch is bound by its
// own latency, not by these bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_play_delay_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = pp::DELAY_BLOCK;
constexpr int kResetBlocks = 1024;                              // the reset's grid-stride cap

__global__ __launch_bounds__(kBlock) void play_delay_push_kernel(const uint32_t* __restrict__ in, int64_t ld_in, const int64_t* __restrict__ done, int32_t rows,
                                                                 int32_t num_agents, int32_t width, int32_t depth, int32_t rows_per_block,
                                                                 const int32_t* __restrict__ delay, int32_t* __restrict__ age, uint32_t* ring,
                                                                 uint32_t* __restrict__ out, int64_t ld_out) {
    __shared__ int32_t slot_write[kBlock], slot_read[kBlock];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;     // < rows: the grid is ceil(rows / rows_per_block)
    const int32_t left = (int32_t)((int64_t)rows - r0);
    const int32_t n = left < rows_per_block ? left : rows_per_block;      // 1 .. kBlock rows
    if (tid < n) {
        const int64_t r = r0 + tid;
        const pp::delay_slots s = pp::delay_index(done, num_agents, r, age[r], delay[r], depth);
        slot_write[tid] = s.write;
        slot_read[tid] = s.read;
        age[r] = s.next;
    }
    __syncthreads();
    const int32_t words = n * width;                             // <= max(1024, 512)
    for (int32_t i = tid; i < words; i += kBlock) {
        const int32_t row = i / width, c = i - row * width;
        pp::delay_move(in, ld_in, ring, out, ld_out, rows, width, r0 + row, c, slot_write[row], slot_read[row]);
    }
}

__global__ __launch_bounds__(kBlock) void play_delay_reset_kernel(int32_t rows, int32_t* __restrict__ age) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) age[i] = 0;
}

}  // namespace

extern "C" size_t pp_play_delay_ring_bytes(int32_t rows, int32_t width, int32_t depth) {
    return pp::delay_ring_bytes(rows, width, depth);
}

extern "C" int pp_play_delay_reset(int32_t rows, int32_t* age, void* stream) {
    if (rows < 1 || !age) {
        pp_set_errorf("pp_play_delay_reset: NULL pointer or rows < 1");
        return PPENV_EINVAL;
    }
    const int64_t blocks = ((int64_t)rows + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(play_delay_reset_kernel, dim3((uint32_t)(blocks < kResetBlocks ? blocks : kResetBlocks)), dim3(kBlock), 0, (hipStream_t)stream, rows, age);
    return pp_launched("launching play_delay_reset_kernel failed");
}

extern "C" int pp_play_delay_push(const float* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width, int32_t depth,
                                  const int32_t* delay, int32_t* age, float* ring, float* out, int64_t ld_out, void* stream) {
    if (!pp::delay_sizes_ok(rows, num_agents, width, depth) || !in || !delay || !age || !ring || !out || ld_in < width || ld_out < width) {
        pp_set_errorf("pp_play_delay_push: NULL pointer (done excepted), rows < 1 or no multiple of num_agents, num_agents not 1 or 2, width outside 1..%d, "
                      "depth outside 1..%d, or a stride below width", PP_PLAY_DELAY_MAX_WIDTH, PP_PLAY_DELAY_MAX + 1);
        return PPENV_EINVAL;
    }
    const int32_t per = pp::delay_rows_per_block(width);
    const int64_t blocks = ((int64_t)rows + per - 1) / per;      // <= rows <= 2^31 - 1
    hipLaunchKernelGGL(play_delay_push_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t*)in, ld_in, done, rows, num_agents,
                       width, depth, per, delay, age, (uint32_t*)ring, (uint32_t*)out, ld_out);
    return pp_launched("launching play_delay_push_kernel failed");
}
