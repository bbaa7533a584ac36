/*
 * ppenv_critic_input.h — C ABI of the PRIVILEGED CRITIC INPUTS of training: the quantities an env hides from the policy — its
 * randomisation tables (ppenv_dr.h, ppenv_dr_adr.h), its control delays (ppenv_train_delay.h), its undelayed observation — gathered
 * into one fp32 row per actor row, and that row normalised into the columns of the first-layer operand that only the critic's weights
 * read (isaacgym_amd.critic_input.CriticInput, RolloutCollector(critic_input=), PPOTrainer(critic_inputs=), python -m isaacgym_amd.ppo
 * --critic-inputs).  An asymmetric actor-critic after OpenAI's ADR (Akkaya et al. 2019) and DeXtreme (Handa et al. 2022).
 *
 * THERE IS NO REFERENCE FOR THIS.  The layout below is this project's own specification; the tests check the kernels against it restated
 * in numpy, and the second kernel against ppenv_mlp_prepare_input on the concatenated row.
 *
 * THE SOURCE TABLE.  1 .. PP_CRITIC_MAX_SOURCES sources, written once on the host and uploaded (pp_critic_input_upload), as the dims of
 * ppenv_dr_adr.h are.  Source s has an element kind (float32 or int32), `cols` columns and one of two layouts, strides in ELEMENTS:
 *
 *     ROW-MAJOR    [rows, cols], element (r, c) at p[r * stride + c], stride >= cols: one row per ACTOR row
 *     TABLE-MAJOR  [cols, num_envs], element (c, e) at p[c * stride + e], stride >= num_envs: a table row is contiguous over ENVS — how the
 *                  randomisation tables are stored; a per-env scalar [num_envs] is one such column
 *
 * `rows` actor rows, num_agents A in {1, 2}, num_envs = rows / A; env e owns rows A * e .. A * e + A - 1, so actor row r reads env
 * e(r) = r / A of a table-major source: ppenv_train_delay.h's map, and both rows of a 4-actor env see the same table columns.
 * The sources' columns follow one another in table order: source s starts at column off_s = cols_0 + .. + cols_{s-1}, and the width of
 * the privileged row is P = the sum of all cols, 1 <= P <= PP_CRITIC_MAX_COLS.
 *
 * GATHER.  out[r][off_s + c] = (float) element (r, c) of a row-major source, or element (c, e(r)) of a table-major one.  A float32
 * element is copied bit for bit; an int32 element is converted as C converts it (round to nearest even beyond 2^24).  Nothing else of
 * `out` is written.  One launch: workgroup (i, s) owns the 64 actor rows 64 i .. 64 i + 63 (the ragged last one guarded) of source s.
 * A row-major source is copied with consecutive lanes on consecutive columns.  A table-major source goes through an LDS tile: lanes
 * run along envs while a table row is read, so every load is coalesced, and along the columns of `out` while it is written.
 *
 * PREPARE.  The second half of preparing a first-layer operand wider than the observation: x16[r][col0 + j] = fp16(clamp((priv[r][j] -
 * mean[j]) * inv_std[j], -clip, clip)) for j < P — ppenv_mlp_prepare_input's arithmetic per element, each operation rounded on its own,
 * then round to nearest even to fp16; with mean and inv_std both NULL the value is only converted — and x16[r][col0 + P .. ld_x16) = 0.
 * The columns below col0 are left as they are.  ppenv_mlp_prepare_input, called with the wide ld_out, writes the observation columns and
 * zeroes every column above its k, so the order is fixed: it runs first, this launch second.  The stores are 16 bytes wide from the
 * first column that is a multiple of 8 on; the up to 7 columns before it (col0 is odd for 313 observations) are stored as elements.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation, no atomics, no sums: a captured launch replays like an eager one.
 * Returns 0 or a negative PPENV_E* code (ppenv.h) with the message in ppenv_last_error().
 */
#ifndef PPENV_CRITIC_INPUT_H
#define PPENV_CRITIC_INPUT_H

#include "ppenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_CRITIC_MAX_SOURCES 16
#define PP_CRITIC_MAX_COLS 1024

#define PP_CRITIC_F32 0                          /* kind: float32 elements */
#define PP_CRITIC_I32 1                          /* kind: int32 elements, converted to float */
#define PP_CRITIC_ROW_MAJOR 0                    /* layout: [rows, cols] */
#define PP_CRITIC_TABLE_MAJOR 1                  /* layout: [cols, num_envs] */

typedef struct pp_critic_source {
    const void* p;                               /* device */
    int32_t kind;                                /* PP_CRITIC_F32 or PP_CRITIC_I32 */
    int32_t cols;                                /* >= 1 */
    int32_t layout;                              /* PP_CRITIC_ROW_MAJOR or PP_CRITIC_TABLE_MAJOR */
    int32_t reserved;
    int64_t stride;                              /* elements: between rows (row-major, >= cols) or between table rows (table-major, >= num_envs) */
} pp_critic_source;

typedef struct pp_critic_table {
    int32_t rows;                                /* actor rows, >= 1 and a multiple of num_agents */
    int32_t num_agents;                          /* 1 or 2 */
    int32_t sources;                             /* 1 .. PP_CRITIC_MAX_SOURCES */
    int32_t total_cols;                          /* P: pp_critic_input_upload computes it */
    pp_critic_source source[PP_CRITIC_MAX_SOURCES];
} pp_critic_table;

/* Validates *table (host memory; its total_cols is ignored), sets total_cols = the sum of the sources' cols and copies the struct to
 * table_dev (sizeof(pp_critic_table) bytes of device memory, 8-byte aligned).  Refuses, naming the field: rows < 1 or no multiple of
 * num_agents, num_agents not 1 or 2, sources outside 1 .. PP_CRITIC_MAX_SOURCES, and per source a NULL pointer, an unknown kind or layout,
 * cols < 1, a stride below cols (row-major) or below rows / num_agents (table-major), or a total above PP_CRITIC_MAX_COLS.  A set-up
 * call: it waits for its copy.  The sources must outlive every later launch.  -> 0, or a negative code. */
int pp_critic_input_upload(const pp_critic_table* table, pp_critic_table* table_dev, void* stream);

/* GATHER.  rows and num_agents must be the uploaded ones (rows sizes the grid; the smaller of the two row counts bounds every access).
 * out [rows, ld_out] float32, ld_out >= P in elements: the caller's own slice, e.g. of a horizon buffer.  One launch. */
int pp_critic_input_gather(const pp_critic_table* table_dev, int32_t rows, int32_t num_agents, float* out, int64_t ld_out, void* stream);

/* PREPARE.  priv [rows, ld_priv] float32, ld_priv >= P; mean, inv_std [P] float32, both or neither; x16 [rows, ld_x16] fp16, 16-byte
 * aligned, ld_x16 a multiple of 8; 0 <= col0 and col0 + P <= ld_x16, 1 <= P <= PP_CRITIC_MAX_COLS.  One launch. */
int pp_critic_input_prepare(const float* priv, int64_t ld_priv, int32_t rows, int32_t P, const float* mean, const float* inv_std, float clip,
                            void* x16, int32_t ld_x16, int32_t col0, void* stream);

#ifdef __cplusplus
}
#endif

#endif
