/*
 * ppenv_ta_outcome.h — C ABI of the 27-dof task's outcome counts: the five head-counts of envs the reference prints, and then
 * zeroes, whenever any env resets (tasks/humanoid_pingpong_3_actor_all_dof.py, "TA", post_physics_step TA:1161-1175):
 * fell down, came close to the paddle, hit the paddle, crossed the net, hit the table.
 *
 * The step kernels keep those events as the PPENV_TA_COUNT_* bits of `flags` (ppenv.h) and clear them, in every env, in the launch
 * of the step in which some env resets — that step's own events included, so the sums cannot be rebuilt afterwards.  With a
 * pp_ta_outcome attached, the workgroup that clears sums the five bits over all envs first and adds the sums to the struct: a
 * "window" is one such clear.  Off (the default) the launches do what they did before, bit for bit.
 *
 * One workgroup writes the struct, and only a later launch reads it: no word a workgroup reads is written by another workgroup in
 * the same launch, so a captured step replays like an eager one.  The sums are integers: any order gives the same bits.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the
 * message in ppenv_last_error().
 */
#ifndef PPENV_TA_OUTCOME_H
#define PPENV_TA_OUTCOME_H

#include <stddef.h>
#include <stdint.h>

#include "ppenv.h"
#include "ppenv_play.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_TA_OUTCOME_COUNTS 5
/* index of a count in pp_ta_outcome.count / .last: the order of the bits 16, 32, 64, 128, 256 of `flags` */
#define PP_TA_OUTCOME_CLOSER 0
#define PP_TA_OUTCOME_HIT_PADDLE 1
#define PP_TA_OUTCOME_CROSS_NET 2
#define PP_TA_OUTCOME_HIT_TABLE 3
#define PP_TA_OUTCOME_FALL_DOWN 4

typedef struct pp_ta_outcome {     /* 128 bytes, device memory, 8-byte aligned, zeroed by the caller */
    uint64_t windows;              /* clears so far: steps in which at least one env reset (TA:1162) */
    uint64_t envs;                 /* sum of num_envs over those steps */
    uint64_t count[PP_TA_OUTCOME_COUNTS];   /* summed over windows: envs whose bit stood right BEFORE the clear, this step's events included;
                                      order of bits 16,32,64,128,256: closer, hit_paddle, cross_net, hit_table, fall_down */
    uint64_t last_envs;            /* the most recent window alone: what the reference's five prints show */
    uint64_t last[PP_TA_OUTCOME_COUNTS];
    uint64_t reserved[3];
} pp_ta_outcome;

/* From the next ppenv_ta_step of this handle on, the launch that clears the count bits adds their sums to *dev first (all three
 * kernels: chain-wave, quad, one lane per env).  dev NULL switches it off.  The struct is read and written by every later step: the
 * caller keeps it alive. */
int pp_ta_sim_set_outcome(ppenv_ta_sim* s, pp_ta_outcome* dev);

/* ppenv_ta_post_physics_step (ppenv.h: the same arguments, the same launches, the same outputs) with the counts summed into
 * *outcome_dev before they are cleared; outcome_dev NULL: exactly ppenv_ta_post_physics_step. */
int pp_ta_post_physics_step_outcome(const ppenv_ta_params* params, const float* rb_states_dev, const float* initial_rb_states_dev,
                                    float* root_states_dev, float* dof_states_dev, const float* dof_force_dev, const float* pre_ball_vx_dev,
                                    const float* reset_override_dev, uint32_t* flags_dev, uint32_t* episode_dev, int64_t* progress_dev,
                                    float* obs_dev, float* rew_dev, int64_t* reset_dev, uint32_t* scratch_any_reset_dev,
                                    pp_ta_outcome* outcome_dev, void* stream);

/* One wave: *latched = *live iff totals->games < games_num when it runs; otherwise nothing changes — the freeze rule of
 * ppenv_play_accumulate (ppenv_play.h).  Launched after an env step and before that step's ppenv_play_accumulate, it leaves in
 * `latched` the counts as they stood after the step at which a host-synchronised loop would have stopped, however rarely the host
 * looks. */
int pp_ta_outcome_latch(const pp_ta_outcome* live, const ppenv_play_totals* totals, int64_t games_num, pp_ta_outcome* latched, void* stream);

#ifdef __cplusplus
}
#endif

#endif
