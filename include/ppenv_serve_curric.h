/*
 * ppenv_serve_curric.h — C ABI of the SERVE CURRICULUM: the serve space cut into bins, every finished game's return credited to the bin
 * its ball was drawn from, every env's next serve drawn from a per-bin probability table that favours the bins the policy scores worst on.
 *
 * The reference has no serve curriculum: the rule below is this project's own specification.  No oracle pins it; the tests check the
 * kernels against the rule restated twice, a host build of csrc/ppenv_serve_curric_device.h and numpy.
 *
 * A curriculum writes the override buffer a serve plan writes (ppenv_serve.h: serve_override [3][N], layout SOA3, or the 27-dof
 * reset_override [N,5], layout AOS5), so the step kernels are untouched.  B bins, 1 <= B <= PP_CURRIC_MAX_BINS, each a pp_serve_cell with
 * the plan's validation (the +-PP_SERVE_MAX_TILT_DEG bound included).
 *
 * Draws.  Serve j of env e, key = env_id_offset + e:
 *     u24  = the 24-bit integer rng_uniform(seed, key, j, 5) scales (its hash chain's h >> 8; index 5 is unused by the plan's 0 .. 4)
 *     bin  = #{ b in 0 .. B-2 : cdf[b] <= u24 }                      (cdf[B-1] == 1 << 24 always)
 *     ball = serve_draw's formula (ppenv_serve.h) with cells[bin] for the group's cell and the same (seed, key, j, 0 .. 4) draws
 *
 * Device state, all caller-allocated, zero = fresh unless noted (pp_serve_curric_state holds the pointers):
 *     per env  count[N] u32 serves consumed; next_bin[N] i32 the bin of the serve now in the override buffer; cur_bin[N] i32 the bin of the
 *              running episode, -1 = not counted (the episode running when the curriculum was installed was served by the built-in draw);
 *              ret[N] f32 the running return
 *     per bin  games[B] i64; mean[B] f32; dropped[B] i64; cdf[B] u32
 *     staging  fin_bin[H][N] i32, fin_q[H][N] i64: one row per control step of a horizon
 *
 * STEP, once per control step after the env step that wrote rew [A*N] and reset [reset_rows*N]; r = A*e is agent 0's row:
 *     ret[e] += rew[r]                                         (unscaled reward, fp32, in this order)
 *     reset[reset_rows*e] != 0 (all 64 bits):
 *         fin_bin_t[e] = cur_bin[e];  fin_q_t[e] = q(ret[e])   (the step that ends a game carries its last reward)
 *         ret[e] = 0;  cur_bin[e] = next_bin[e]                (the reset just consumed the buffer's row)
 *         j = ++count[e];  next_bin[e] = bin(e, j);  out[e] = serve(e, j) from cells[next_bin[e]]
 *     else fin_bin_t[e] = -1                                   (out, count and the bins are untouched, bit for bit)
 *     q(x) = (int64_t)((double)x * 65536.0), truncating; a return that is not finite or beyond 2^31 in magnitude is staged as
 *     PP_CURRIC_DROPPED and counted in dropped[bin], not in games or mean.  Sums of q values are integer sums: one value in any order.
 *
 * FOLD, once per horizon: tot[3][B] i64 = per bin the games n, the sum q of fin_q, the dropped games d over the count staged entries
 * (bin -1 skipped).  Integer adds only: the same bits whatever the grid.
 *
 * UPDATE, once per epoch, on tot (summed over data-parallel ranks by the caller):
 *     n_b > 0:  m = (float)((double)q_b / (65536.0 * (double)n_b))
 *               mean[b] = games[b] == 0 ? m : mean[b] + alpha * (m - mean[b]);  games[b] += n_b;       dropped[b] += d_b (always)
 *     rank_b = 1 + #{ c : games[c] > 0 && (mean[c] < mean[b] || (mean[c] == mean[b] && c < b)) }   for a seen bin (1 = lowest mean return)
 *     rank_b = 1                                                                                    for an unseen bin: tried first
 *     w_b = 1, then `power` times w_b *= 1.0 / (double)rank_b
 *     p_b = (1 - mix) * w_b / W + mix / B,   W = w_0 + w_1 + ... in bin order, all in double
 *     cdf[b] = (uint32)floor(16777216.0 * (p_0 + ... + p_b)), summed in bin order;  cdf[B-1] = 1 << 24
 * power == 0 or mix == 1: uniform bins, a curriculum that only keeps the statistics (the control run).
 * The update runs between two horizons, in stream order with the steps that read cdf.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation, no global atomics; nothing but sizes travels by value, so a captured
 * launch replays like an eager one.  Returns 0 or a negative PPENV_E* code (ppenv.h), the text in ppenv_last_error().  Compiled unfused
 * (-ffp-contract=off), as ppenv_serve.hip is, so that the host build gives the same bits.
 */
#ifndef PPENV_SERVE_CURRIC_H
#define PPENV_SERVE_CURRIC_H

#include "ppenv_serve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_CURRIC_MAX_BINS 256
#define PP_CURRIC_MAX_POWER 4
#define PP_CURRIC_RNG_INDEX 5u                   /* the draw index of the bin */
#define PP_CURRIC_DROPPED INT64_MIN              /* fin_q of a game whose return cannot be credited */
#define PP_CURRIC_FOLD_CHUNK 16384               /* staged entries per workgroup of the fold */

typedef struct pp_serve_curric {
    int32_t num_envs;
    int32_t env_id_offset;                       /* global id of env 0 (>= 0) */
    uint64_t seed;                               /* a STREAM seed, keyed as given */
    int32_t form;                                /* PPENV_VARIANT_* for serve_from_draws */
    int32_t layout;                              /* PP_SERVE_LAYOUT_* */
    int32_t reset_rows;                          /* rows of reset per env: 1 or 2 */
    int32_t num_agents;                          /* rows of rew per env: 1 or 2 (row A e, agent 0's, is credited) */
    int32_t bins;                                /* B */
    int32_t power;                               /* 0 .. PP_CURRIC_MAX_POWER */
    float mix;                                   /* [0, 1]: the uniform share of every bin */
    float alpha;                                 /* (0, 1]: the weight of a horizon's mean in mean[b] */
    const pp_serve_cell* cells;                  /* device, [bins] */
} pp_serve_curric;

typedef struct pp_serve_curric_state {           /* device pointers; the struct itself is host memory */
    uint32_t* count;
    int32_t* next_bin;
    int32_t* cur_bin;
    float* ret;
    int64_t* games;
    float* mean;
    int64_t* dropped;
    uint32_t* cdf;
} pp_serve_curric_state;

/* Mirrors pp_serve_plan_upload and refuses what it refuses (with groups = 1); also bins outside 1 .. PP_CURRIC_MAX_BINS, num_agents not
 * 1 or 2, power outside 0 .. PP_CURRIC_MAX_POWER, mix outside [0, 1], alpha outside (0, 1], either non-finite.  cells_dev: bins *
 * sizeof(pp_serve_cell) bytes; curric_dev: sizeof(pp_serve_curric) bytes, 8-byte aligned.  A set-up call: it waits for its copies. */
int pp_serve_curric_upload(const pp_serve_curric* curric, const pp_serve_cell* cells, pp_serve_curric* curric_dev, pp_serve_cell* cells_dev, void* stream);

/* cdf = the uniform table ((b + 1) << 24) / B; for every env next_bin[e] = bin(e, count[e]), out[e] = serve(e, count[e]), cur_bin[e] = -1,
 * ret[e] = 0.  num_envs and bins must be the uploaded ones (they size the grid; the smaller of each pair bounds every access). */
int pp_serve_curric_fill(const pp_serve_curric* curric_dev, int32_t num_envs, int32_t bins, const pp_serve_curric_state* state, float* out, void* stream);

/* STEP.  fin_bin_t [N] i32 and fin_q_t [N] i64: the caller's row t of the staging buffers. */
int pp_serve_curric_step(const pp_serve_curric* curric_dev, int32_t num_envs, const float* rew, const int64_t* reset, const pp_serve_curric_state* state,
                         float* out, int32_t* fin_bin_t, int64_t* fin_q_t, void* stream);

/* Bytes of the fold's workspace for `count` staged entries (0 when count <= 0): one [3][PP_CURRIC_MAX_BINS] i64 row per workgroup. */
size_t pp_serve_curric_fold_bytes(int64_t count);

/* FOLD over fin_bin [count], fin_q [count] (count = H * N, contiguous) -> tot [3][bins] i64 (n, q, d), overwritten.  Workgroup w sums
 * entries [w * PP_CURRIC_FOLD_CHUNK, ...) into its own row of `partial` with integer adds in LDS; a second, one-workgroup kernel of the
 * same call adds the rows in workgroup order.  With one workgroup the first kernel writes tot itself.  Entries whose bin is outside
 * [0, bins) are skipped. */
int pp_serve_curric_fold(const int32_t* fin_bin, const int64_t* fin_q, int64_t count, int32_t bins, int64_t* tot, void* partial, void* stream);

/* UPDATE: one workgroup, lane b per bin. */
int pp_serve_curric_update(const pp_serve_curric* curric_dev, int32_t bins, const int64_t* tot, const pp_serve_curric_state* state, void* stream);

#ifdef __cplusplus
}
#endif

#endif
