// ppenv_history.hip — the observation and action history of the actor on the device (include/ppenv_history.h).
//
//   history_push_kernel   workgroup b owns the rows [b * R, b * R + R), R = pp::history_rows_per_block(W) (the ragged last workgroup
//                         guarded).  Lane t < R reads row t's done word (pp::history_start) and leaves `start` in LDS; after the barrier the
//                         256 lanes walk the workgroup's R * pp::history_pieces(W) 16-byte pieces of `next` in order, consecutive lanes on
//                         consecutive pieces of one row (pp::history_move_piece: one 16-byte load and store where source and destination are
//                         both 16-byte aligned inside one slot run, element accesses otherwise and at the row's two edges).
// A pure copy: per row W words written and W read (n on a start).  No atomics, no counter on the host: a push is a function of its
// arguments alone, so a captured launch replays like an eager one.  A workgroup writes `next` of its own rows only and reads nothing
// another writes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_history_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = pp::HISTORY_BLOCK;

__global__ __launch_bounds__(kBlock) void history_push_kernel(const uint32_t* __restrict__ obs, int64_t ld_obs, const uint32_t* __restrict__ act, int64_t ld_act,
                                                              const int64_t* __restrict__ done, const uint32_t* prev, int64_t ld_prev, uint32_t* next,
                                                              int64_t ld_next, int32_t rows, int32_t num_agents, pp::history_shape s, int32_t rows_per_block,
                                                              float lo, float hi) {
    __shared__ int32_t start_of[kBlock];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;     // < rows: the grid is ceil(rows / rows_per_block)
    const int32_t left = (int32_t)((int64_t)rows - r0);
    const int32_t n = left < rows_per_block ? left : rows_per_block;      // 1 .. kBlock rows
    if (tid < n) start_of[tid] = pp::history_start(prev != nullptr, done, num_agents, r0 + tid) ? 1 : 0;
    __syncthreads();
    const int32_t pieces = pp::history_pieces(s.W);
    const int32_t total = n * pieces;                            // <= max(1024, pieces)
    for (int32_t i = tid; i < total; i += kBlock) {
        const int32_t row = i / pieces, p = i - row * pieces;
        const int64_t r = r0 + row;
        pp::history_move_piece(obs + r * ld_obs, act ? act + r * ld_act : nullptr, prev ? prev + r * ld_prev : nullptr, next + r * ld_next, s, start_of[row] != 0,
                               p, lo, hi);
    }
}

}  // namespace

extern "C" int32_t pp_history_width(int32_t n, int32_t A, int32_t Ho, int32_t Ha) { return pp::history_width(n, A, Ho, Ha); }

extern "C" int pp_history_push(const float* obs, int64_t ld_obs, const float* act, int64_t ld_act, const int64_t* done, const float* prev, int64_t ld_prev,
                               float* next, int64_t ld_next, int32_t rows, int32_t num_agents, int32_t n, int32_t A, int32_t Ho, int32_t Ha, float lo, float hi,
                               void* stream) {
#define PP_HISTORY_REFUSE(cond, ...)                   \
    do {                                               \
        if (cond) {                                    \
            pp_set_errorf("pp_history_push: " __VA_ARGS__); \
            return PPENV_EINVAL;                       \
        }                                              \
    } while (0)
    PP_HISTORY_REFUSE(!obs, "obs is NULL");
    PP_HISTORY_REFUSE(!next, "next is NULL");
    PP_HISTORY_REFUSE(num_agents != 1 && num_agents != 2, "num_agents %d is not 1 or 2", num_agents);
    PP_HISTORY_REFUSE(rows < 1 || rows % num_agents, "rows %d < 1 or no multiple of num_agents %d", rows, num_agents);
    PP_HISTORY_REFUSE(Ho < 0 || Ho > PP_HISTORY_MAX, "Ho %d outside 0..%d", Ho, PP_HISTORY_MAX);
    PP_HISTORY_REFUSE(Ha < 0 || Ha > PP_HISTORY_MAX, "Ha %d outside 0..%d", Ha, PP_HISTORY_MAX);
    PP_HISTORY_REFUSE(Ho == 0 && Ha == 0, "Ho and Ha are both 0: there is no history");
    PP_HISTORY_REFUSE(n < 1, "n %d < 1", n);
    PP_HISTORY_REFUSE(A < 1, "A %d < 1", A);
    const int64_t wide = (int64_t)(Ho + 1) * n + (int64_t)Ha * A;
    PP_HISTORY_REFUSE(wide > PP_HISTORY_MAX_WIDTH, "W %lld > %d", (long long)wide, PP_HISTORY_MAX_WIDTH);
    PP_HISTORY_REFUSE(ld_obs < n, "ld_obs %lld < n %d", (long long)ld_obs, n);
    PP_HISTORY_REFUSE(act && ld_act < A, "ld_act %lld < A %d", (long long)ld_act, A);
    PP_HISTORY_REFUSE(prev && ld_prev < wide, "ld_prev %lld < W %lld", (long long)ld_prev, (long long)wide);
    PP_HISTORY_REFUSE(ld_next < wide, "ld_next %lld < W %lld", (long long)ld_next, (long long)wide);
    PP_HISTORY_REFUSE(!(lo <= hi), "lo %g > hi %g", (double)lo, (double)hi);
    PP_HISTORY_REFUSE((const float*)next == prev, "next == prev: the two rows must not alias");
    PP_HISTORY_REFUSE(!act && prev && Ha > 0, "act is NULL with a prev and Ha %d > 0", Ha);
#undef PP_HISTORY_REFUSE
    const pp::history_shape s = {n, A, Ho, Ha, (int32_t)wide};
    const int32_t per = pp::history_rows_per_block(s.W);
    const int64_t blocks = ((int64_t)rows + per - 1) / per;      // <= rows <= 2^31 - 1
    hipLaunchKernelGGL(history_push_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t*)obs, ld_obs, (const uint32_t*)act, ld_act,
                       done, (const uint32_t*)prev, ld_prev, (uint32_t*)next, ld_next, rows, num_agents, s, per, lo, hi);
    return pp_launched("launching history_push_kernel failed");
}
