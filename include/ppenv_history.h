/*
 * ppenv_history.h — C ABI of the OBSERVATION AND ACTION HISTORY of the actor: a frame stack kept on the device.  The policy's input row
 * becomes the observation it sees now, the Ho observations it saw before and its own last Ha commands, so that a memoryless MLP can
 * infer what training under control latency (ppenv_train_delay.h) and randomisation (ppenv_dr.h, ppenv_dr_adr.h) hide from a single
 * observation: a per-episode delay, a link mass (isaacgym_amd.history.HistoryStack, RolloutCollector(history=), PPOTrainer(history=),
 * python -m isaacgym_amd.ppo --obs-history / --action-history; a played checkpoint brings its own record).  Memory by frame stacking, as
 * the policies of OpenAI's ADR (Akkaya et al. 2019) and DeXtreme (Handa et al. 2022) are given memory.
 *
 * THERE IS NO REFERENCE FOR THIS.  Like the delay lines, the rule below is this project's own specification; the tests check the kernel
 * against it restated in numpy, bit for bit.
 *
 * THE WIDE ROW.  A history is (Ho, Ha): Ho earlier observations and Ha earlier actions, each 0 .. PP_HISTORY_MAX, at least one of them
 * positive.  With n the env's observation width and A its action width, in 32-bit words,
 *
 *     W    = (Ho + 1) * n + Ha * A                       <= PP_HISTORY_MAX_WIDTH
 *     wide = [ o_0 | o_1 | .. | o_Ho | a_1 | .. | a_Ha ]
 *
 * o_0 is the observation the policy sees now (under a sensing delay line: the delayed one), o_k the one it saw k control steps ago, a_j
 * the policy's own command of j control steps ago, clamped to [lo, hi] — what the collector stores and the player's policy returns, not
 * what a command delay line made the env consume.
 *
 * THE PUSH.  One push per control step builds `next` from `prev`, the new observation `obs`, the action `act` the policy issued on
 * `prev`, and that step's `done`.  `rows` actor rows, num_agents in {1, 2}; actor row r belongs to env e = r / num_agents:
 *
 *     start = (prev == NULL) || (done != NULL && done[num_agents * e] != 0)      all 64 bits of agent 0's word: the delay lines' rule
 *     o_0 = obs[r]
 *     start:      o_k = obs[r] for every k (hold the first sample, as the delay lines do);  a_j = 0 for every j
 *     otherwise:  o_k = prev.o_{k-1} (k >= 1);  a_1 = fminf(fmaxf(act[r], lo), hi);  a_j = prev.a_{j-1} (j >= 2)
 *
 * Nothing is carried across a reset.  Every word of next[r][0 .. W) is written and nothing beyond W.  Observation words and the words
 * taken from prev are copied bit for bit, NaN payloads included.  The state IS the previous wide row: no ring, no age table, no counter
 * on the host — a push is a function of its arguments alone, so a captured launch replays like an eager one.  prev and next never alias.
 *
 * One launch.  A workgroup owns whole rows; one lane per row reads `done`, then all lanes walk the rows' output in 16-byte pieces of
 * `next`.  A piece is moved as one 16-byte word where it lies inside one slot run and its source is 16-byte aligned too, and as
 * elements otherwise, so the kernel is correct at every 4-byte alignment of rows and slots (n = 313 on the 27-dof task).
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation, no atomics.  Returns 0 or a negative PPENV_E* code (ppenv.h) with
 * the message in ppenv_last_error().
 */
#ifndef PPENV_HISTORY_H
#define PPENV_HISTORY_H

#include "ppenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_HISTORY_MAX 8                         /* Ho and Ha: 0 .. 8 */
#define PP_HISTORY_MAX_WIDTH 16256               /* W: what the input-statistics kernel allows for k */

/* W = (Ho + 1) * n + Ha * A, or 0 for what pp_history_push refuses: n < 1, A < 1, Ho or Ha outside 0 .. PP_HISTORY_MAX, both zero,
 * or W > PP_HISTORY_MAX_WIDTH. */
int32_t pp_history_width(int32_t n, int32_t A, int32_t Ho, int32_t Ha);

/* obs [rows, ld_obs >= n], act [rows, ld_act >= A], prev [rows, ld_prev >= W], next [rows, ld_next >= W]: float32, strides in elements;
 * done [rows] int64.  prev and done may be NULL; act may be NULL only when prev is NULL or Ha == 0.  Refused with PPENV_EINVAL before any
 * device call, naming the field: NULL obs or next, rows < 1 or no multiple of num_agents, num_agents not 1 or 2, Ho or Ha outside
 * 0 .. PP_HISTORY_MAX, both zero, n < 1, A < 1, a stride below its width, W > PP_HISTORY_MAX_WIDTH, lo > hi, next == prev, and a NULL act
 * where it is read.  One launch. */
int pp_history_push(const float* obs, int64_t ld_obs, const float* act, int64_t ld_act, const int64_t* done, const float* prev, int64_t ld_prev,
                    float* next, int64_t ld_next, int32_t rows, int32_t num_agents, int32_t n, int32_t A, int32_t Ho, int32_t Ha, float lo, float hi,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif
