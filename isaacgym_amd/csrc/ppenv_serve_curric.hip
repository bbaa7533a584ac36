// ppenv_serve_curric.hip — the serve curriculum on the device (include/ppenv_serve_curric.h): bins of serve ranges, each finished game
// credited to its ball's bin, each next serve drawn from a table that favours the bins with the lowest mean return.
//
// The reference has no serve curriculum: the rule is this project's own specification (the header states it), unpinned by any oracle.
//
// fill / step are streaming kernels in the shape of ppenv_serve.hip: one lane per env, PP_SERVE_BLOCK envs per workgroup, the ragged tail
// guarded.  Every per-env word (count, next_bin, cur_bin, ret, the env's part of `out`, its staging entries) belongs to lane e alone; cdf
// is read-only in the step and written by the fill's workgroup 0 (which draws from the same table computed, not read) and by the update.
// A step's idle lane reads ret, rew and reset, writes ret and its fin_bin word, all coalesced.
//
// fold: workgroup w owns PP_CURRIC_FOLD_CHUNK consecutive staged entries and a [3][256] i64 table in LDS (6 KB); its lanes stride over the
// chunk (coalesced 4-byte reads; the 8-byte fin_q is read for finished games only, a few per cent of the entries) and add into LDS with
// ds_add_u64 — integer adds, the sum is the same in any order.  The table goes to the workgroup's own row of `partial`, and a second,
// one-workgroup kernel adds the rows in workgroup order, lane b per bin.  With one workgroup the first kernel writes tot itself.
//
// update: one workgroup of 256 lanes, lane b per bin, four phases through LDS (games / mean, w, p; 7 KB).  The sums over bins are
// sequential loops in bin order, as the rule states them: 256 fp64 adds per lane at most, once per epoch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_serve_curric_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kBlock = PP_SERVE_BLOCK;
constexpr int kBins = PP_CURRIC_MAX_BINS;
static_assert(kBlock == kBins, "one lane per bin: the fill's first workgroup, the fold's LDS table, the update");

__global__ __launch_bounds__(kBlock) void curric_fill_kernel(const pp_serve_curric* __restrict__ C, int32_t n_arg, int32_t b_arg, pp_serve_curric_state S,
                                                             float* __restrict__ out) {
    const int32_t B = min(b_arg, C->bins);
    if (blockIdx.x == 0 && (int32_t)threadIdx.x < B) S.cdf[threadIdx.x] = pp::curric_uniform_cdf(B, (int32_t)threadIdx.x);
    const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (e >= n_arg || e >= C->num_envs) return;
    pp::curric_fill_env(*C, B, e, S, out);
}

__global__ __launch_bounds__(kBlock) void curric_step_kernel(const pp_serve_curric* __restrict__ C, int32_t n_arg, const float* __restrict__ rew,
                                                             const int64_t* __restrict__ reset, pp_serve_curric_state S, float* __restrict__ out,
                                                             int32_t* __restrict__ fin_bin_t, int64_t* __restrict__ fin_q_t) {
    const int32_t e = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (e >= n_arg || e >= C->num_envs) return;
    pp::curric_step_env(*C, e, rew, reset, S, out, fin_bin_t, fin_q_t);
}

// dst: row blockIdx.x of [grid][3][stride] (the workspace, stride kBins; or tot itself, grid 1 and stride bins)
__global__ __launch_bounds__(kBlock) void curric_fold_kernel(const int32_t* __restrict__ fin_bin, const int64_t* __restrict__ fin_q, int64_t count, int32_t bins,
                                                             int64_t* __restrict__ dst, int32_t stride) {
    __shared__ unsigned long long acc[3][kBins];
    for (int k = 0; k < 3; ++k) acc[k][threadIdx.x] = 0ull;            // kBlock == kBins lanes
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * PP_CURRIC_FOLD_CHUNK;
    const int64_t hi = lo + PP_CURRIC_FOLD_CHUNK < count ? lo + PP_CURRIC_FOLD_CHUNK : count;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
        const int32_t bin = fin_bin[i];
        if (bin < 0 || bin >= bins) continue;
        const int64_t q = fin_q[i];
        const int kind = pp::curric_fold_kind(bin, q, bins);
        if (kind == 0) {
            atomicAdd(&acc[0][bin], 1ull);
            atomicAdd(&acc[1][bin], (unsigned long long)q);
        } else {
            atomicAdd(&acc[2][bin], 1ull);
        }
    }
    __syncthreads();
    if ((int32_t)threadIdx.x < bins) {
        int64_t* row = dst + (size_t)blockIdx.x * 3u * (size_t)stride;
        for (int k = 0; k < 3; ++k) row[(size_t)k * stride + threadIdx.x] = (int64_t)acc[k][threadIdx.x];
    }
}

__global__ __launch_bounds__(kBlock) void curric_fold_tail_kernel(const int64_t* __restrict__ partial, int32_t rows, int32_t bins, int64_t* __restrict__ tot) {
    const int32_t b = (int32_t)threadIdx.x;
    if (b >= bins) return;
    for (int k = 0; k < 3; ++k) {
        int64_t s = 0;
        for (int32_t w = 0; w < rows; ++w) s += partial[((size_t)w * 3u + k) * kBins + b];
        tot[(size_t)k * bins + b] = s;
    }
}

__global__ __launch_bounds__(kBlock) void curric_update_kernel(const pp_serve_curric* __restrict__ C, int32_t b_arg, const int64_t* __restrict__ tot,
                                                               pp_serve_curric_state S) {
    __shared__ int64_t games[kBins];
    __shared__ float mean[kBins];
    __shared__ double w[kBins], p[kBins];
    const int32_t B = min(b_arg, C->bins), b = (int32_t)threadIdx.x;
    const bool live = b < B;
    if (live) {
        pp::curric_ema_bin(*C, B, b, tot, S.games, S.mean, S.dropped);
        games[b] = S.games[b];
        mean[b] = S.mean[b];
    }
    __syncthreads();
    if (live) w[b] = pp::curric_weight_bin(*C, B, b, games, mean);
    __syncthreads();
    if (live) p[b] = pp::curric_prob_bin(*C, B, b, w);
    __syncthreads();
    if (live) S.cdf[b] = pp::curric_cdf_bin(B, b, p);
}

bool state_ok(const pp_serve_curric_state* s) {
    return s && s->count && s->next_bin && s->cur_bin && s->ret && s->games && s->mean && s->dropped && s->cdf;
}

inline int64_t fold_rows(int64_t count) { return (count + PP_CURRIC_FOLD_CHUNK - 1) / PP_CURRIC_FOLD_CHUNK; }

}  // namespace

extern "C" int pp_serve_curric_upload(const pp_serve_curric* c, const pp_serve_cell* cells, pp_serve_curric* curric_dev, pp_serve_cell* cells_dev, void* stream) {
    if (!c || !cells || !curric_dev || !cells_dev) {
        ppenv_set_error("pp_serve_curric_upload: NULL pointer");
        return PPENV_EINVAL;
    }
    if (const int why = pp::curric_invalid(*c, cells)) {
        static const char* const text[] = {"", "num_envs < 1", "env_id_offset < 0", "unknown form (a PPENV_VARIANT_* value)", "unknown layout", "reset_rows not 1 or 2",
                                           "a cell with a non-finite value or lo > hi", "a tilt or tilt_z bound beyond +-57 degrees (the short sine / cosine series)",
                                           "bins outside 1 .. 256", "num_agents not 1 or 2", "power outside 0 .. 4",
                                           "mix outside [0, 1] or alpha outside (0, 1], or one of them not finite"};
        pp_set_errorf("pp_serve_curric_upload: %s", text[why]);
        return PPENV_EINVAL;
    }
    pp_serve_curric host = *c;
    host.cells = cells_dev;
    if (hipMemcpyAsync(cells_dev, cells, (size_t)c->bins * sizeof(pp_serve_cell), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipMemcpyAsync(curric_dev, &host, sizeof(pp_serve_curric), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {                    // set-up, once: `host` lives on this stack
        (void)hipGetLastError();
        ppenv_set_error("pp_serve_curric_upload: copying the curriculum to the device failed");
        return PPENV_EHIP;
    }
    return PPENV_OK;
}

extern "C" int pp_serve_curric_fill(const pp_serve_curric* curric_dev, int32_t num_envs, int32_t bins, const pp_serve_curric_state* state, float* out, void* stream) {
    if (!curric_dev || !state_ok(state) || !out || num_envs <= 0 || bins < 1 || bins > kBins) {
        ppenv_set_error("pp_serve_curric_fill: NULL pointer, num_envs <= 0 or bins outside 1 .. 256");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(curric_fill_kernel, dim3(pp_blocks_of(num_envs, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, curric_dev, num_envs, bins, *state, out);
    return pp_launched("launching curric_fill_kernel failed");
}

extern "C" int pp_serve_curric_step(const pp_serve_curric* curric_dev, int32_t num_envs, const float* rew, const int64_t* reset, const pp_serve_curric_state* state,
                                    float* out, int32_t* fin_bin_t, int64_t* fin_q_t, void* stream) {
    if (!curric_dev || !rew || !reset || !state_ok(state) || !out || !fin_bin_t || !fin_q_t || num_envs <= 0) {
        ppenv_set_error("pp_serve_curric_step: NULL pointer or num_envs <= 0");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(curric_step_kernel, dim3(pp_blocks_of(num_envs, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, curric_dev, num_envs, rew, reset, *state, out,
                       fin_bin_t, fin_q_t);
    return pp_launched("launching curric_step_kernel failed");
}

extern "C" size_t pp_serve_curric_fold_bytes(int64_t count) {
    return count <= 0 ? 0 : (size_t)fold_rows(count) * 3u * kBins * sizeof(int64_t);
}

extern "C" int pp_serve_curric_fold(const int32_t* fin_bin, const int64_t* fin_q, int64_t count, int32_t bins, int64_t* tot, void* partial, void* stream) {
    if (!fin_bin || !fin_q || !tot || count <= 0 || bins < 1 || bins > kBins || fold_rows(count) > INT32_MAX || (fold_rows(count) > 1 && !partial)) {
        ppenv_set_error("pp_serve_curric_fold: NULL pointer, count <= 0 or bins outside 1 .. 256");
        return PPENV_EINVAL;
    }
    const int32_t rows = (int32_t)fold_rows(count);
    if (rows == 1) {
        hipLaunchKernelGGL(curric_fold_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, fin_bin, fin_q, count, bins, tot, bins);
        return pp_launched("launching curric_fold_kernel failed");
    }
    hipLaunchKernelGGL(curric_fold_kernel, dim3(rows), dim3(kBlock), 0, (hipStream_t)stream, fin_bin, fin_q, count, bins, (int64_t*)partial, kBins);
    hipLaunchKernelGGL(curric_fold_tail_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const int64_t*)partial, rows, bins, tot);
    return pp_launched("launching curric_fold_kernel failed");
}

extern "C" int pp_serve_curric_update(const pp_serve_curric* curric_dev, int32_t bins, const int64_t* tot, const pp_serve_curric_state* state, void* stream) {
    if (!curric_dev || !tot || !state_ok(state) || bins < 1 || bins > kBins) {
        ppenv_set_error("pp_serve_curric_update: NULL pointer or bins outside 1 .. 256");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(curric_update_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, curric_dev, bins, tot, *state);
    return pp_launched("launching curric_update_kernel failed");
}
