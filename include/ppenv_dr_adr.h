/*
 * ppenv_dr_adr.h — C ABI of AUTOMATIC DOMAIN RANDOMISATION (ADR): a device-resident curriculum over the RANGES of reset-time domain
 * randomisation (ppenv_dr.h).  Every randomised table has a current range [lo, hi]; a share of the envs play a whole game pinned to one
 * boundary of one table; finished games are credited to that boundary; once per epoch every boundary whose games score at or above
 * t_high moves outward and every boundary whose games score at or below t_low moves back in.  After OpenAI's ADR (Akkaya et al. 2019) and
 * DeXtreme (Handa et al. 2022); the reference's task map lists an AllegroHandADR, its code has none.
 *
 * The rule below is this project's own specification.  No oracle pins it; the tests check the kernels against the rule restated twice, a
 * host build of csrc/ppenv_dr_adr_device.h and numpy.
 *
 * Dims.  D dims, 1 <= D <= PPENV_DR_MAX_TABLES; dim d is one of the SoA [rows][num_envs] tables the step kernels read by pointer, rows in
 * 1 .. PPENV_DR_MAX_ROWS.  A dim is always a uniform SCALING without schedule (ppenv_dr.h's vocabulary).  Per dim, by value: start_lo,
 * start_hi (the range a fresh run draws from), limit_lo, limit_hi (how far it may widen) and step (how far one update moves a boundary),
 * with 0 < limit_lo <= start_lo <= start_hi <= limit_hi and step > 0, all finite.
 *
 * Slots.  S = 2 D + 1.  Slot 2 d + s is side s (0 = lo, 1 = hi) of dim d; slot 2 D is "interior": a game played with every table drawn
 * inside its range.
 *
 * Device state, all caller-allocated, zero = fresh unless noted (pp_dr_adr_state holds the pointers):
 *     per dim   range[D][2] f32: the current lo, hi (FILL sets them to the starts)
 *     per env   draws[N] i32 redraws the env has had; slot[N] i32 the slot of the running game, -1 = not credited; ret[N] f32 its return
 *     per slot  acc_n[S], acc_q[S] i64 games and summed q since the slot was last judged; games[S], dropped[S] i64 all games ever;
 *               mean[S] f32 the mean return it was last judged on; widened[S], narrowed[S] i32 the moves it has made
 *     staging   fin_slot[H][N] i32, fin_q[H][N] i64: one row per control step of a horizon
 *
 * DRAW(e, j) under ranges (lo_d, hi_d), gid = env_id_offset + e, sd = seed ^ PPENV_DR_SEED_SALT (dr_base's key):
 *     table d, row r = dr_shape(rng_uniform(sd, gid, j, dr_key(d, r)), UNIFORM, SCALING, lo_d, hi_d, 1.0f)
 *                      — the bits ppenv_dr_apply writes for a plan of these ranges (dr_key(d, r) = d * PPENV_DR_MAX_ROWS + r)
 *     c24 = the 24-bit integer rng_uniform(sd, gid, j, PP_ADR_COIN_INDEX) scales (its hash chain's h >> 8); index 512 =
 *           PPENV_DR_MAX_TABLES * PPENV_DR_MAX_ROWS is the first index no table row uses
 *     c24 < thr: the env is a BOUNDARY WORKER.  p24 likewise from PP_ADR_PICK_INDEX (513); b = (p24 * 2 D) >> 24 in 64 bits; every row of
 *           table b >> 1 is overwritten with the stored lo (b & 1 == 0) or hi (b & 1 == 1) ITSELF, bit for bit; slot = b
 *     otherwise slot = 2 D
 * Consecutive lanes are consecutive envs of one row: every store instruction is coalesced, as in dr_redraw.
 *
 * FILL:  range = the starts; every env: j = draws[e]++, columns of DRAW(e, j) under the starts, slot[e] = -1 (the running game began
 *     under other tables and is not credited), ret[e] = 0.
 *
 * STEP, once per control step after the env step that wrote rew [A * N] (unscaled) and reset [reset_rows * N] i64, all 64 bits tested:
 *     ret[e] += rew[A * e]                                                  (agent 0's row, fp32)
 *     reset[reset_rows * e] != 0:
 *         fin_slot_t[e] = slot[e];  fin_q_t[e] = q(ret[e]);  ret[e] = 0     (the step that ends a game carries its last reward)
 *         j = draws[e]++;  (columns, slot[e]) = DRAW(e, j) under range[] as it stands
 *     else fin_slot_t[e] = -1                                               (nothing else of env e changes, bit for bit)
 *     Every reset redraws: there is no `frequency` here.  q is the serve curriculum's (ppenv_serve_curric.h): 16.16 fixed point,
 *     truncating; a return that is not finite or beyond 2^31 in magnitude is staged as PP_CURRIC_DROPPED.
 *
 * FOLD, once per horizon: pp_serve_curric_fold (ppenv_serve_curric.h) on fin_slot / fin_q with bins = S -> tot[3][S] i64 (games n, sum
 *     q, dropped d).  It is generic over (bin, q) pairs; there is no second fold.
 *
 * UPDATE, once per epoch, on tot (summed over data-parallel ranks by the caller), per slot s:
 *     games[s] += n;  dropped[s] += d;  acc_n[s] += n;  acc_q[s] += q
 *     acc_n[s] >= min_games:
 *         m = (float)((double)acc_q[s] / (65536.0 * (double)acc_n[s]));  mean[s] = m
 *         a boundary slot with m >= t_high WIDENS:   lo = fmaxf(lo - step, limit_lo)   or   hi = fminf(hi + step, limit_hi);  widened[s] += 1
 *         else one with m <= t_low NARROWS:          lo = fminf(lo + step, start_lo)   or   hi = fmaxf(hi - step, start_hi);  narrowed[s] += 1
 *         acc_n[s] = acc_q[s] = 0                    (in all three cases; the interior slot only keeps its mean)
 *     Each fp32 operation rounds on its own.  lo <= start_lo <= start_hi <= hi holds after every update; both sides of a dim may move in
 *     one update.  (With t_low == t_high a mean equal to both widens.)
 * A game is credited to the slot it was DRAWN for: the boundary value it ran at may be one update older than the current one, since the
 * update runs between two horizons (in stream order with the steps that read range[]) while games straddle them.
 *
 * Degenerate settings.  boundary_frac = 0: fixed-range randomisation by this kernel, the control run.  t_high = +FLT_MAX, t_low =
 * -FLT_MAX: the statistics only.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation, no global atomics; nothing but sizes travels by value, so a captured
 * launch replays like an eager one.  Returns 0 or a negative PPENV_E* code (ppenv.h), the text in ppenv_last_error().  Compiled unfused
 * (-ffp-contract=off), so that the host build gives the same bits.
 */
#ifndef PPENV_DR_ADR_H
#define PPENV_DR_ADR_H

#include "ppenv_dr.h"
#include "ppenv_serve_curric.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ADR_COIN_INDEX 512u                   /* PPENV_DR_MAX_TABLES * PPENV_DR_MAX_ROWS: the boundary coin's draw index */
#define PP_ADR_PICK_INDEX 513u                   /* the draw index of the boundary a worker is pinned to */
#define PP_ADR_MAX_SLOTS (2 * PPENV_DR_MAX_TABLES + 1)

typedef struct pp_dr_adr_dim {
    float* table;                                /* device, [rows][num_envs] */
    int32_t rows;                                /* 1 .. PPENV_DR_MAX_ROWS */
    float start_lo, start_hi, limit_lo, limit_hi, step;
} pp_dr_adr_dim;

typedef struct pp_dr_adr {
    int32_t num_envs;
    int32_t env_id_offset;                       /* global id of env 0 (>= 0) */
    uint64_t seed;                               /* a STREAM seed, keyed as given */
    int32_t reset_rows;                          /* rows of reset per env: 1 or 2 */
    int32_t num_agents;                          /* rows of rew per env: 1 or 2 (row A e, agent 0's, is credited) */
    int32_t dims;                                /* D */
    uint32_t thr;                                /* floor(boundary_frac * 2^24): pp_dr_adr_upload computes it */
    int32_t min_games;                           /* >= 1: games a slot must have gathered before it is judged */
    float t_low, t_high;                         /* t_low <= t_high, finite */
    int32_t reserved;
    pp_dr_adr_dim dim[PPENV_DR_MAX_TABLES];
} pp_dr_adr;

typedef struct pp_dr_adr_state {                 /* device pointers; the struct itself is host memory */
    float* range;
    int32_t* draws;
    int32_t* slot;
    float* ret;
    int64_t* acc_n;
    int64_t* acc_q;
    int64_t* games;
    int64_t* dropped;
    float* mean;
    int32_t* widened;
    int32_t* narrowed;
} pp_dr_adr_state;

/* Validates *adr (host memory; its thr is ignored) and boundary_frac, sets thr = floor(boundary_frac * 2^24) computed in double, and
 * copies the struct to adr_dev (sizeof(pp_dr_adr) bytes of device memory, 8-byte aligned).  Refuses, naming the field: num_envs < 1,
 * env_id_offset < 0, reset_rows or num_agents not 1 or 2, dims outside 1 .. PPENV_DR_MAX_TABLES, boundary_frac outside [0, 1] or not
 * finite, min_games < 1, t_low / t_high not finite or t_low > t_high, and per dim a NULL table, rows outside 1 .. PPENV_DR_MAX_ROWS, a
 * non-finite value, step <= 0, limit_lo <= 0, or anything violating limit_lo <= start_lo <= start_hi <= limit_hi.  A set-up call: it
 * waits for its copy.  The tables must outlive every later launch. */
int pp_dr_adr_upload(const pp_dr_adr* adr, double boundary_frac, pp_dr_adr* adr_dev, void* stream);

/* FILL.  num_envs and dims must be the uploaded ones (they size the grid; the smaller of each pair bounds every access). */
int pp_dr_adr_fill(const pp_dr_adr* adr_dev, int32_t num_envs, int32_t dims, const pp_dr_adr_state* state, void* stream);

/* STEP.  fin_slot_t [N] i32 and fin_q_t [N] i64: the caller's row t of the staging buffers.  An env that does not reset costs the reads
 * of ret, rew and reset and the writes of ret and its fin_slot word, in two dependent memory round trips. */
int pp_dr_adr_step(const pp_dr_adr* adr_dev, int32_t num_envs, const float* rew, const int64_t* reset, const pp_dr_adr_state* state,
                   int32_t* fin_slot_t, int64_t* fin_q_t, void* stream);

/* UPDATE: one workgroup, lane s per slot; tot [3][2 * dims + 1] i64. */
int pp_dr_adr_update(const pp_dr_adr* adr_dev, int32_t dims, const int64_t* tot, const pp_dr_adr_state* state, void* stream);

#ifdef __cplusplus
}
#endif

#endif
