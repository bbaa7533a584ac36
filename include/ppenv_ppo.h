/*
 * ppenv_ppo.h — C ABI of the PPO minibatch tail: rl_games' a2c_continuous losses and their gradient, the gradient-norm clip, PyTorch's
 * Adam and GradScaler's dynamic loss scale, all on the device (cfg/train/HumanoidPingpongTiltG1PPO.yaml:50-85: e_clip, critic_coef,
 * clip_value, bounds_loss_coef, entropy_coef, grad_norm, truncate_grads, mixed_precision, learning_rate).
 *
 * Per minibatch step, after the learner's forward:
 *   ppenv_ppo_loss_grad      d(loss x scale) / d [mu | value] per row (what NativeMLPLearner.backward takes), d(loss x scale) / d logstd,
 *                            and the minibatch means of the loss terms, KL and clip fraction (two launches: per-row work with one
 *                            partial row per workgroup, then a fixed-order sum of the partial rows by one workgroup)
 *   (the learner's backward)
 *   ppenv_ppo_grad_sumsq     per-workgroup partial sums of the squared, still scaled gradients of every tensor in a table
 *   ppenv_ppo_adam_step      every workgroup sums the partials in the same order; unscale, clip, Adam; a non-finite norm skips the step
 *                            (with ppenv_ppo_adam.world > 1: on the rank means of all-reduced gradient sums); the loss scale stays
 *                            within bounds (ppenv_ppo_scaler, below)
 *
 * No float atomics anywhere: every sum has a fixed order, so results are bitwise reproducible run to run.  The loss scale and the
 * step count live in a ppenv_ppo_scaler on the device and are never read by the host: ppenv_ppo_adam_step reads `state_in` and writes
 * the next state to `state_out`, a DIFFERENT struct (every workgroup reads the state; none rewrites what the others read in the same
 * launch).  The caller alternates the two buffers.
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the
 * message in ppenv_last_error().
 */
#ifndef PPENV_PPO_H
#define PPENV_PPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPENV_PPO_MAX_ACTIONS 32       /* one lane per row holds the row's actions */
#define PPENV_PPO_PARTIAL_STRIDE 40    /* floats per partial row: d logstd [32], then a_loss, c_loss, b_loss, kl, clipped */
#define PPENV_PPO_MAX_TENSORS 64

/* stats[] written by ppenv_ppo_loss_grad: minibatch means, unscaled */
enum { PPENV_PPO_LOSS = 0, PPENV_PPO_A_LOSS, PPENV_PPO_C_LOSS, PPENV_PPO_B_LOSS, PPENV_PPO_ENTROPY, PPENV_PPO_KL, PPENV_PPO_CLIP_FRAC, PPENV_PPO_NUM_STATS = 8 };

typedef struct ppenv_ppo_loss_args {
    int32_t m, a;                                   /* rows of the minibatch, actions (a <= 32) */
    const float* mu;          int32_t ld_mu;        /* [m, ld_mu] the heads' output, columns 0 .. a-1 */
    const float* value;       int32_t ld_value;     /* [m, ld_value] column 0 (normalised value space with normalize_value) */
    const float* actions;     int32_t ld_actions;   /* [m, ld_actions] the stored actions */
    const float* old_mu;      int32_t ld_old_mu;    /* [m, ld_old_mu] the rollout's mu (KL) */
    const float* old_sigma;                         /* [a] the rollout's sigma (KL) */
    const float* old_neglogp;                       /* [m] */
    const float* advantages;                        /* [m] normalised */
    const float* old_values;                        /* [m] */
    const float* returns;                           /* [m] */
    const float* logstd;                            /* [a] */
    float e_clip, critic_coef, bounds_loss_coef, soft_bound, entropy_coef;
    int32_t clip_value;                             /* 1: clipped value loss (clip_value: True) */
    const float* scale;                             /* device scalar: the loss scale (ppenv_ppo_scaler.scale) */
    float* d_head;            int32_t ld_d_head;    /* out [m, ld_d_head]: columns 0 .. a-1 d/d mu, column a d/d value; x scale */
    float* d_logstd;                                /* out [a] x scale */
    float* stats;                                   /* out [PPENV_PPO_NUM_STATS] */
    float* partial;                                 /* workspace: ppenv_ppo_loss_partial_floats(m) floats */
} ppenv_ppo_loss_args;

size_t ppenv_ppo_loss_partial_floats(int32_t m);
int ppenv_ppo_loss_grad(const ppenv_ppo_loss_args* args, void* stream);

/* One tensor of the optimizer: p [rows, cols] with row stride ld_p, its gradient with row stride ld_g, the moments contiguous [rows, cols].
 * 16-byte vector accesses where cols, both strides and every pointer allow them; element accesses otherwise. */
typedef struct ppenv_ppo_tensor {
    float* p; const float* g; float* m; float* v;
    int32_t rows, cols, ld_p, ld_g;
} ppenv_ppo_tensor;

/* GradScaler's state (torch.cuda.amp.GradScaler: init_scale, growth_tracker) and the optimizer's step count.
 *
 * The scale is BOUNDED, a deliberate departure from torch's GradScaler, which bounds neither end (a long burst of overflowing steps halves
 * torch's scale down to 0, and the first clean step after it divides by that 0):
 *   - a dynamic scale (backoff_factor < 1) never leaves ppenv_ppo_adam_step below PPENV_PPO_SCALE_FLOOR, the scale a run without mixed
 *     precision has throughout; below it a scale only shrinks the gradients ahead of their fp16 cast.  A state found below the floor (a
 *     checkpoint of a run that had none) is lifted to it by its next update, skipped or clean; reserved[0] counts the updates the floor
 *     changed;
 *   - growth is withheld (growth_tracker still restarts) where scale x growth_factor is not finite;
 *   - a step whose scale is not a normal positive number (0, a denormal, negative, NaN: nothing finite divides it out) is skipped like a step
 *     with a non-finite norm, so finite gradients never put a non-finite value into a parameter or a moment.
 * With a constant scale (factors 1.0) and at every scale in [1, 2^126] the arithmetic of a step is unchanged. */
#define PPENV_PPO_SCALE_FLOOR 1.0f

typedef struct ppenv_ppo_scaler {
    float scale;
    int32_t growth_tracker;    /* clean steps since the last change of the scale */
    int32_t step;              /* Adam steps taken (skipped steps do not count) */
    int32_t skipped;           /* steps skipped: a non-finite gradient norm, or a scale that cannot be divided out */
    float grad_norm;           /* the unscaled gradient norm of the last step (before the clip) */
    int32_t reserved[3];       /* [0]: updates in which the floor changed the scale; [1], [2]: 0 */
} ppenv_ppo_scaler;

typedef struct ppenv_ppo_adam {
    double beta1, beta2;       /* torch.optim.Adam defaults: 0.9, 0.999 (fp64 as torch has them: 1 - beta2 and the bias corrections are
                                  formed from the double, the moment updates use its fp32 rounding) */
    float eps;                 /* 1e-8 */
    float max_norm;            /* grad_norm */
    int32_t truncate;          /* truncate_grads: clip_grad_norm_(max_norm) */
    float growth_factor, backoff_factor;   /* 2.0, 0.5 (1.0, 1.0: a constant scale) */
    int32_t growth_interval;   /* 2000 */
    int32_t world;             /* data-parallel ranks; 0 or 1: one.  Above 1 the gradient buffers hold the SUMS over the ranks (each x the loss
                                  scale, as a gradient all-reduce leaves them): Adam consumes fl(g_sum / world), a correctly rounded fp32 division
                                  (rl_games' all_grads / world_size), then unscales; the norm, the clip and the skip are those of these means */
} ppenv_ppo_adam;

/* table: `count` ppenv_ppo_tensor in DEVICE memory (written once by the caller).  parts: the workgroups of both launches and the length
 * of `slab` (fp64); the same value must be passed to both. */
int ppenv_ppo_grad_sumsq(const ppenv_ppo_tensor* table, int32_t count, double* slab, int32_t parts, void* stream);
int ppenv_ppo_adam_step(const ppenv_ppo_tensor* table, int32_t count, const double* slab, int32_t parts, ppenv_ppo_adam hp, const float* lr,
                        const ppenv_ppo_scaler* state_in, ppenv_ppo_scaler* state_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
