/*
 * ppenv_serve.h — C ABI of the SERVE PLAN: each env's next serve, kept on the device in the override buffer its step kernel reads.
 *
 * Every step-kernel family has a per-env override that a reset consumes instead of its RNG: the 7-dof and 4-actor handles read
 * ppenv_buffers.serve_override [3][N] while ppenv_set_serve_override(h, NULL, 1) is on (step_kernel*, init_kernel, reset_idx_kernel);
 * ppenv_ta_step takes reset_override [N,5] = ball y, z, v_x, v_y, v_z.  A plan says what those buffers hold: env e belongs to group
 * e / envs_per_group, its group's CELL gives the range of every serve quantity (lo == hi pins one), and
 *     serve(e, j):   u_k = rng_uniform(seed, key(e), j, k),    k = 0 speed, 1 tilt, 2 tilt_z, 3 ball_y, 4 ball_z
 *                    quantity = lo + (hi - lo) * u             (the T3 form ignores tilt_z; layout 0 ignores k = 3, 4)
 *                    velocity = serve_from_draws(form, speed, tilt, tilt_z)       (isaacgym_amd/csrc/ppenv_device.h, the step kernels' own)
 *     key(e) = env_id_offset + e   (paired == 0: an env's serves are the same whatever the shard)
 *            = e % envs_per_group  (paired == 1: env i of EVERY group is served the same sequence of balls — common random numbers)
 * `seed` keys the draws as given: a STREAM seed (ppenv.h "What a seed means here"); the tasks pass scene.stream_seed(seed, STREAM_SERVES),
 * a family of its own, so no draw is shared with the built-in serves, the step noise, the tables or the sampler.
 *
 * State: one caller-allocated uint32 count[N] on the device, all zeros when fresh: the serves env e has consumed.  The buffer always
 * holds serve(e, count[e]).  There are no shared scalars, so a launch captured in a HIP graph replays correctly by construction.
 *
 * Graphs.  The 7-dof handles' override SWITCH travels by value in the step kernel's arguments: a graph captured before the switch was
 * turned on (or off) does not see the change and must be captured again.  The launches below take pointers only and can be captured.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation, no atomics; returns 0 or a negative PPENV_E* code (ppenv.h)
 * with the message in ppenv_last_error().  The unit is compiled unfused (-ffp-contract=off) so that a host build of
 * csrc/ppenv_serve_device.h gives the same bits, serve_from_draws as instantiated in this unit included (the step kernels' own
 * contracted copy of that function need not agree with it in the last bit, and nothing requires it to).
 */
#ifndef PPENV_SERVE_H
#define PPENV_SERVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_SERVE_BLOCK 256                 /* envs per workgroup */
#define PP_SERVE_MAX_TILT_DEG 57.0f        /* what ppenv_create refuses beyond: the short sine / cosine series of serve_from_draws */

enum { PP_SERVE_LAYOUT_SOA3 = 0,           /* out [3][N]: v_x, v_y, v_z           (ppenv_buffers.serve_override) */
       PP_SERVE_LAYOUT_AOS5 = 1 };         /* out [N,5]:  ball y, z, v_x, v_y, v_z (ppenv_ta_step's reset_override) */

typedef struct pp_serve_cell {             /* lo == hi pins a quantity */
    float speed_lo, speed_hi, tilt_lo_deg, tilt_hi_deg, tilt_z_lo_deg, tilt_z_hi_deg, ball_y_lo, ball_y_hi, ball_z_lo, ball_z_hi;
} pp_serve_cell;

typedef struct pp_serve_plan {
    int32_t num_envs;
    int32_t env_id_offset;                 /* global id of env 0 (>= 0) */
    uint64_t seed;                         /* a STREAM seed, keyed as given */
    int32_t form;                          /* PPENV_VARIANT_* for serve_from_draws (the 27-dof task passes PPENV_VARIANT_TN) */
    int32_t layout;                        /* PP_SERVE_LAYOUT_* */
    int32_t reset_rows;                    /* rows of reset_buf per env: 1; 2 for the 4-actor variant (row 2 e is read) */
    int32_t groups, envs_per_group;        /* groups * envs_per_group == num_envs */
    int32_t paired;                        /* 0 / 1: the key, above */
    const pp_serve_cell* cells;            /* device, [groups] */
} pp_serve_plan;

/* Validates *plan and cells[plan->groups] (host memory), copies the cells to cells_dev (groups * sizeof(pp_serve_cell) bytes) and the plan,
 * pointing at them, to plan_dev (sizeof(pp_serve_plan) bytes, 8-byte aligned).  A set-up call: the copies go through `stream` and the call
 * waits for them.  Refused (PPENV_EINVAL): a tilt or tilt_z bound beyond +-PP_SERVE_MAX_TILT_DEG, lo > hi, a non-finite value,
 * groups * envs_per_group != num_envs (or any of them < 1), env_id_offset < 0, an unknown form or layout, reset_rows not 1 or 2, paired
 * not 0 or 1. */
int pp_serve_plan_upload(const pp_serve_plan* plan, const pp_serve_cell* cells, pp_serve_plan* plan_dev, pp_serve_cell* cells_dev, void* stream);

/* out[e] = serve(e, count[e]) for every env; nothing advances.  num_envs must be the uploaded plan's (it sizes the grid; the smaller
 * of the two bounds every access). */
int pp_serve_fill(const pp_serve_plan* plan_dev, int32_t num_envs, float* out, const uint32_t* count, void* stream);

/* One control step, launched after the step that produced reset_buf ([reset_rows * num_envs] int64).  For each env e whose word
 * reset_buf[reset_rows * e] is non-zero (all 64 bits): count[e] += 1; out[e] = serve(e, count[e]).  Every other env is left
 * untouched, bit for bit; it costs its one reset_buf read. */
int pp_serve_apply(const pp_serve_plan* plan_dev, int32_t num_envs, const int64_t* reset_buf, float* out, uint32_t* count, void* stream);

/* The same body for a list of DISTINCT local env ids (reset_idx(env_ids)): each listed env has consumed its serve.  Ids outside
 * [0, num_envs) are skipped.  env_ids: int64, device. */
int pp_serve_apply_ids(const pp_serve_plan* plan_dev, int32_t num_envs, const int64_t* env_ids, int32_t n_ids, float* out, uint32_t* count,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif
