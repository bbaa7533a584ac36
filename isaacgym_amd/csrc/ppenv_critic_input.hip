// ppenv_critic_input.hip — the privileged critic inputs on the device (include/ppenv_critic_input.h).
//
//   critic_gather_kernel    workgroup (i, s) owns the actor rows [64 i, 64 i + 64) of source s (the ragged last tile guarded; a workgroup whose s
//                           is beyond the uploaded table's sources leaves at once: the grid is sized for PP_CRITIC_MAX_SOURCES, since the table
//                           lives on the device).  A row-major source is copied with the 256 lanes walking the tile's words in order: consecutive
//                           lanes on consecutive columns of one row, on both sides.  A table-major source is transposed through an LDS tile of
//                           64 rows x 64 columns (row pitch 65 words, so neither side has a bank conflict): wave w reads the table rows w, w + 4,
//                           .. with its lanes along the 64 actor rows — consecutive envs (each twice for a 4-actor env), one coalesced load — and
//                           after the barrier the lanes walk the tile by rows of `out`.
//   critic_prepare_kernel   one lane per 8 output columns from the 16-byte piece that holds col0 on: every load is unconditional (clamped
//                           index), the piece is stored as one 16-byte word, or as elements where it begins below col0.
// No atomics and no sums; a workgroup writes its own rows and columns only and reads nothing another writes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_critic_input_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = pp::CRITIC_BLOCK, kRows = pp::CRITIC_TILE_ROWS, kCols = pp::CRITIC_TILE_COLS;

__global__ __launch_bounds__(kBlock) void critic_gather_kernel(const pp_critic_table* __restrict__ T, int32_t rows_arg, float* __restrict__ out, int64_t ld_out) {
    __shared__ float tile[kRows][kCols + 1];
    const int32_t s = (int32_t)blockIdx.y, tid = (int32_t)threadIdx.x;
    if (s >= T->sources) return;                                 // uniform over the workgroup, like every branch around a barrier below
    const int32_t rows = rows_arg < T->rows ? rows_arg : T->rows, A = T->num_agents;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    if (r0 >= rows) return;
    const int32_t n = rows - r0 < kRows ? (int32_t)(rows - r0) : kRows;
    int64_t off = 0;
    for (int32_t k = 0; k < s; k++) off += T->source[k].cols;
    const pp_critic_source src = T->source[s];
    const int64_t room = ld_out - off;                           // a row of `out` narrower than the table's P is never overrun
    const int32_t cols = room < src.cols ? (int32_t)(room < 0 ? 0 : room) : src.cols;
    if (src.layout == PP_CRITIC_ROW_MAJOR) {
        const int32_t words = n * cols;                          // <= 64 * 1024
        for (int32_t i = tid; i < words; i += kBlock) {
            const int32_t row = i / cols, c = i - row * cols;
            out[(r0 + row) * ld_out + off + c] = pp::critic_element(src, A, r0 + row, c);
        }
        return;
    }
    const int32_t lane = tid & 63, wave = tid >> 6;
    for (int32_t c0 = 0; c0 < cols; c0 += kCols) {
        const int32_t w = cols - c0 < kCols ? cols - c0 : kCols;
        if (lane < n)
            for (int32_t cc = wave; cc < w; cc += kBlock / 64) tile[lane][cc] = pp::critic_element(src, A, r0 + lane, c0 + cc);
        __syncthreads();
        for (int32_t i = tid; i < n * w; i += kBlock) {
            const int32_t row = i / w, cc = i - row * w;
            out[(r0 + row) * ld_out + off + c0 + cc] = tile[row][cc];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void critic_prepare_kernel(const float* __restrict__ priv, int64_t ld_priv, int32_t rows, int32_t P, const float* __restrict__ mean,
                                                                const float* __restrict__ inv_std, float clip, _Float16* __restrict__ x16, int32_t ld_x16, int32_t col0) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const int32_t ch0 = col0 >> 3, nch = (ld_x16 >> 3) - ch0;      // >= 1: col0 < ld_x16
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (int64_t)rows * nch) return;
    const int64_t row = idx / nch;
    const int32_t c8 = (ch0 + (int32_t)(idx - row * nch)) * 8;
    const float* p = priv + row * ld_priv;
    h8 v;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int32_t j = c8 + q - col0, jj = j < 0 ? 0 : j < P ? j : P - 1;
        float g = p[jj];
        if (mean) g = pp::critic_normalise(g, mean[jj], inv_std[jj], clip);
        v[q] = j >= 0 && j < P ? (_Float16)g : (_Float16)0.f;
    }
    _Float16* dst = x16 + row * ld_x16 + c8;
    if (c8 >= col0) {
        *reinterpret_cast<h8*>(dst) = v;
    } else {
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (c8 + q >= col0) dst[q] = v[q];
    }
}

}  // namespace

extern "C" int pp_critic_input_upload(const pp_critic_table* table, pp_critic_table* table_dev, void* stream) {
    if (!table || !table_dev) {
        ppenv_set_error("pp_critic_input_upload: NULL pointer");
        return PPENV_EINVAL;
    }
    int32_t which = -1, total = 0;
    if (const int why = pp::critic_table_invalid(*table, &which, &total)) {
        static const char* const text[] = {"", "rows < 1 or no multiple of num_agents", "num_agents not 1 or 2", "sources outside 1 .. 16", "a NULL pointer",
                                           "kind is not 0 (float32) or 1 (int32)", "layout is not 0 (row-major) or 1 (table-major)", "cols outside 1 .. 1024",
                                           "a stride below cols (row-major) or below rows / num_agents (table-major)", "more than 1024 columns in all"};
        if (which >= 0)
            pp_set_errorf("pp_critic_input_upload: source %d: %s", which, text[why]);
        else
            pp_set_errorf("pp_critic_input_upload: %s", text[why]);
        return PPENV_EINVAL;
    }
    pp_critic_table host = *table;
    host.total_cols = total;
    if (hipMemcpyAsync(table_dev, &host, sizeof(pp_critic_table), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {                    // set-up, once: `host` lives on this stack
        (void)hipGetLastError();
        ppenv_set_error("pp_critic_input_upload: copying the table to the device failed");
        return PPENV_EHIP;
    }
    return PPENV_OK;
}

extern "C" int pp_critic_input_gather(const pp_critic_table* table_dev, int32_t rows, int32_t num_agents, float* out, int64_t ld_out, void* stream) {
    if (!table_dev || !out || rows < 1 || (num_agents != 1 && num_agents != 2) || rows % num_agents || ld_out < 1) {
        ppenv_set_error("pp_critic_input_gather: NULL pointer, rows < 1 or no multiple of num_agents, num_agents not 1 or 2, or ld_out < 1");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(critic_gather_kernel, dim3(pp_blocks_of(rows, kRows), PP_CRITIC_MAX_SOURCES), dim3(kBlock), 0, (hipStream_t)stream, table_dev, rows, out,
                       ld_out);
    return pp_launched("launching critic_gather_kernel failed");
}

extern "C" int pp_critic_input_prepare(const float* priv, int64_t ld_priv, int32_t rows, int32_t P, const float* mean, const float* inv_std, float clip,
                                       void* x16, int32_t ld_x16, int32_t col0, void* stream) {
    if (!priv || !x16 || rows < 1 || P < 1 || P > PP_CRITIC_MAX_COLS || ld_priv < P || col0 < 0 || ld_x16 < 8 || (ld_x16 & 7) || (int64_t)col0 + P > ld_x16 ||
        (reinterpret_cast<uintptr_t>(x16) & 15) || ((mean == nullptr) != (inv_std == nullptr))) {
        ppenv_set_error("pp_critic_input_prepare: NULL pointer or inconsistent sizes (need rows >= 1, 1 <= P <= 1024, ld_priv >= P, col0 >= 0, col0 + P <= ld_x16, "
                        "ld_x16 a multiple of 8, x16 16-byte aligned, mean and inv_std together)");
        return PPENV_EINVAL;
    }
    const int64_t pieces = (int64_t)rows * ((ld_x16 >> 3) - (col0 >> 3));
    hipLaunchKernelGGL(critic_prepare_kernel, dim3(pp_blocks_of(pieces, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, priv, ld_priv, rows, P, mean, inv_std, clip,
                       reinterpret_cast<_Float16*>(x16), ld_x16, col0);
    return pp_launched("launching critic_prepare_kernel failed");
}
