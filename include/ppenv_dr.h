/*
 * ppenv_dr.h — C ABI of reset-time, per-env domain randomisation drawn on the device.
 *
 * The reference redraws an env's actor parameters WHEN THAT ENV RESETS: _reset_idx(env_ids) calls apply_randomizations
 * (tasks/humanoid_pingpong_3_actor_tilt.py:849-850), post_physics_step runs `randomize_buf += 1` every step (TT:1025), and upstream
 * VecTask.apply_randomizations redraws the envs with `reset_buf != 0 and randomize_buf >= frequency` — all envs the first time it
 * runs — and zeroes randomize_buf for exactly those.  An episode runs under one set of masses, gains, friction and restitution.
 *
 * A PLAN says what to draw: up to PPENV_DR_MAX_TABLES of the SoA [rows][num_envs] tables the step kernels read by pointer
 * (ppenv_randomization, ppenv.h; the 27-dof task's [27][N] / [28][N] / [N] ones alike), each with the yaml's vocabulary
 * (cfg/task/HumanoidPingpongTiltG1.yaml:100-169): distribution, operation, range, schedule.  One launch per control step applies it:
 * column e of every table is rewritten in place when env e redraws and is not touched otherwise.
 *
 * The numbers come from the library's counter RNG (rng_uniform, isaacgym_amd/csrc/ppenv_device.h) under a key of this path's own:
 *     rng_uniform(seed ^ PPENV_DR_SEED_SALT, env_id_offset + e, draws[e], k),     k = table index * PPENV_DR_MAX_ROWS + row
 * where draws[e] counts the redraws env e has had.  An env's j-th redraw is therefore the same numbers whatever the shard, the
 * launch order or the number of envs, and it never meets the serve or the noise stream.  A Gaussian entry takes Box-Muller on the
 * draws (k & ~1, k | 1): rows 2 j and 2 j + 1 of a table share one pair and take its cosine and its sine branch, the pairing of
 * the noise path.  Its logarithm and sine / cosine are fixed polynomials in fused multiply-adds (ppenv_dr_device.h), so the device
 * and a host build of the same header give the same bits.
 *
 * Everything the launch reads and advances — the control-step count the schedules depend on, the first-application flag (= no
 * step counted yet) and draws[N] — lives in a caller-allocated device block, the STATE, so that a launch captured in a HIP graph
 * stays correct on replay.  All zeros is the fresh state.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation, no float atomics; returns 0 or a negative PPENV_E* code
 * (ppenv.h) with the message in ppenv_last_error().
 */
#ifndef PPENV_DR_H
#define PPENV_DR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPENV_DR_MAX_TABLES 8
#define PPENV_DR_MAX_ROWS 64                          /* rows of one table (the largest in use: 28 link masses) */
#define PPENV_DR_BLOCK 256                            /* envs per workgroup; one step counter per workgroup (see ppenv_dr_state_bytes) */
#define PPENV_DR_SEED_SALT 0xD1B54A32D192ED03ull

enum { PPENV_DR_UNIFORM = 0, PPENV_DR_GAUSSIAN = 1 };                             /* `range` = (lo, hi) / (mu, sigma) */
enum { PPENV_DR_SCALING = 0, PPENV_DR_ADDITIVE = 1 };                             /* blended towards 1 / towards 0 by the schedule weight */
enum { PPENV_DR_SCHED_NONE = 0, PPENV_DR_SCHED_LINEAR = 1, PPENV_DR_SCHED_CONSTANT = 2 };
/* schedule weight at control step t (upstream VecTask.apply_randomizations):
 *   none 1;  linear min(t, schedule_steps) / schedule_steps;  constant t > schedule_steps ? 1 : 0
 * value written = draw * w + (1 - w) for a scaling, draw * w for an additive term (each product and sum rounded to fp32, unfused). */

typedef struct ppenv_dr_entry {
    float* table;              /* device, [rows][num_envs] */
    int32_t rows;              /* 1 .. PPENV_DR_MAX_ROWS */
    int32_t distribution, operation, schedule;
    float a, b;                /* range */
    int32_t schedule_steps;    /* > 0 with a linear schedule, >= 0 with a constant one */
    int32_t reserved;
} ppenv_dr_entry;

typedef struct ppenv_dr_plan {
    int32_t num_envs;
    int32_t env_id_offset;     /* global id of env 0 (ppenv_config.env_id_offset) */
    uint64_t seed;             /* keys the draws as given: a stream seed (ppenv.h "What a seed means here"; the tasks pass the tables' own) */
    int32_t frequency;         /* >= 1: control steps an env must have run since its last redraw before a reset redraws it */
    int32_t reset_rows;        /* rows of reset_buf per env: 1; 2 for the 4-actor variant, whose two agent rows reset together (row 2 e is read) */
    int32_t num_tables;        /* 1 .. PPENV_DR_MAX_TABLES */
    int32_t reserved;
    ppenv_dr_entry entry[PPENV_DR_MAX_TABLES];
} ppenv_dr_plan;

/* Size of the state block for a plan of num_envs envs (0 when num_envs <= 0), and where draws[num_envs] (int32) starts in it.  The
 * block begins with one int64 control-step count per workgroup of PPENV_DR_BLOCK envs: every workgroup keeps a copy of its own
 * (all equal), reads it, meets at a barrier and only then has one lane write the next value — so no workgroup reads a word that
 * another one rewrites in the same launch, with one launch and no atomics.  Fresh state = all bytes zero. */
size_t ppenv_dr_state_bytes(int32_t num_envs);
size_t ppenv_dr_state_draws_offset(int32_t num_envs);

/* Validates *plan (host memory) and copies it to plan_dev (sizeof(ppenv_dr_plan) bytes of device memory, 8-byte aligned).  A
 * set-up call, made once: the copy goes through `stream` and — unlike the launches below — the call waits for it, so the host
 * struct may be dropped when it returns.  The tables named by the plan must outlive every later apply. */
int ppenv_dr_plan_upload(const ppenv_dr_plan* plan, ppenv_dr_plan* plan_dev, void* stream);

/* One control step of the rule, launched after the step that produced reset_buf.  Per env e, in this order:
 *     randomize_buf[e] += 1                                                                (TT:1025)
 *     if this is the first application, or reset_buf[reset_rows * e] != 0 and randomize_buf[e] >= frequency:
 *         redraw column e of every table; randomize_buf[e] = 0; draws[e] += 1
 * then the control-step count advances.  The schedules see the count INCLUDING this step.  An env that does not redraw costs one
 * reset_buf read and one randomize_buf read-modify-write.  reset_buf [reset_rows * num_envs], randomize_buf [num_envs]: int64.
 * num_envs must be the uploaded plan's: it sizes the grid and bounds randomize_buf and the state block (made for that many envs); the
 * plan's own num_envs bounds the table columns, so a mismatch cannot write outside either. */
int ppenv_dr_apply(const ppenv_dr_plan* plan_dev, int32_t num_envs, const int64_t* reset_buf, int64_t* randomize_buf, void* state_dev,
                   void* stream);

/* The same for an explicit list of DISTINCT local env ids (VecTask.reset_idx(env_ids) -> _reset_idx, TT:809-812): a listed env
 * counts as resetting.  It is not a control step: randomize_buf is not incremented and the step count (hence the
 * first-application flag) does not advance.  Per listed e: if no step has been counted yet, or randomize_buf[e] >= frequency:
 * redraw column e, randomize_buf[e] = 0, draws[e] += 1.  Ids outside [0, num_envs) are skipped.  env_ids: int64, device. */
int ppenv_dr_apply_ids(const ppenv_dr_plan* plan_dev, int32_t num_envs, const int64_t* env_ids, int32_t count, int64_t* randomize_buf,
                       void* state_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif
