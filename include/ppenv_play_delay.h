/*
 * ppenv_play_delay.h — C ABI of the CONTROL-LATENCY delay line of a played checkpoint: a per-row delay of whole control steps on a device
 * ring, one for the command path (the policy's actions reach the env d steps late) and one for the sensing path (the policy sees the
 * observation of d steps ago) (isaacgym_amd.play: Delay, Player(action_delay=, obs_delay=), the sweep axes action_delay / obs_delay).
 *
 * THERE IS NO REFERENCE FOR THIS.  The rule below is this build's own specification: nothing in the project this one is modelled on
 * delays a command or an observation, so no oracle pins it; the tests check the kernel against the rule restated twice (a host build of
 * the index arithmetic, and array copies in numpy).
 *
 * A CHANNEL has `rows` actor rows (num_agents * num_envs; env e owns rows A * e .. A * e + A - 1, A = num_agents 1 or 2) of `width` W
 * 32-bit values, a delay d[r] per row in 0 .. K - 1, a ring [K][rows][W] (value (k, r, c) at word (k * rows + r) * W + c) and an age[r]
 * (int32), with K = `depth` = max(d) + 1 <= PP_PLAY_DELAY_MAX + 1.
 *
 * THE RULE.  One push per control step takes in [rows, >= W], an optional done [rows] and out [rows, >= W].  Per row r:
 *
 *     a = (done != NULL && done[A * (r / A)] != 0) ? 0 : age[r]      this sample is the first of a new episode
 *     ring[a % K][r][:] = in[r][:]
 *     s = a - min(a, d[r])                                           max(a - d, 0): the line is primed with the episode's first sample
 *     out[r][:] = ring[s % K][r][:]                                  a bitwise copy; s == a gives in[r]
 *     age[r] = a + 1
 *
 * `done` is the WHOLE 64-bit word of agent 0's row of the env, as in ppenv_play_group.h: both rows of a 4-actor env restart together, and
 * agent 1's word is not read.  pp_play_delay_reset zeroes age; the first push after it passes done = NULL.
 *
 * From sample d of an episode on, every output is exactly d control steps old; before that the episode's FIRST sample is held: a pipeline
 * that starts empty has nothing better to show, and no artificial "neutral" command is invented.  Nothing is carried across a reset: a
 * slot is never read before it was written in the running episode (s <= a, and a - s <= d < K), which is also why the ring need not be
 * cleared.  Values are moved as bits: NaN payloads and -0.0 survive.
 *
 * One launch per push: a workgroup owns a run of whole rows (a row never spans two workgroups); one lane per row reads age[r] — the only
 * read of it — forms the two slots and writes age[r]; after a barrier the workgroup's lanes walk the rows' words in order, consecutive
 * lanes on consecutive words of a row (coalesced whatever W and the strides are).  No atomics, no host-side counter, no word read by one
 * workgroup and written by another in the same launch: a launch captured in a graph replays like an eager one.  The index arithmetic is
 * isaacgym_amd/csrc/ppenv_play_delay_device.h, which the tests also compile for the host.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the message in
 * ppenv_last_error().  Refused with PPENV_EINVAL before any device call: a NULL pointer (`done` excepted), rows < 1, rows no multiple of
 * num_agents, num_agents not 1 or 2, width outside 1..PP_PLAY_DELAY_MAX_WIDTH, depth outside 1..PP_PLAY_DELAY_MAX + 1, a stride (ld_in,
 * ld_out) below width.  A delay[r] >= depth is the CALLER's error and is not looked for on the device (isaacgym_amd.play.Delay checks the
 * table on the host when it uploads it).
 */
#ifndef PPENV_PLAY_DELAY_H
#define PPENV_PLAY_DELAY_H

#include "ppenv_play_group.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_PLAY_DELAY_MAX 15                          /* the largest delay, in control steps: depth <= 16 */
#define PP_PLAY_DELAY_MAX_WIDTH 512

/* Bytes of `ring` (4 * depth * rows * width); 0 for sizes the entries refuse. */
size_t pp_play_delay_ring_bytes(int32_t rows, int32_t width, int32_t depth);

/* age[0 .. rows) to zero.  One launch.  The ring is left as it is. */
int pp_play_delay_reset(int32_t rows, int32_t* age, void* stream);

/* One control step.  in [rows, ld_in] and out [rows, ld_out]: 32-bit values, strides in ELEMENTS, `in` is not modified and must not
 * overlap out or ring; done [rows] int64 or NULL; delay [rows] int32 on the device, every value < depth; age [rows] int32;
 * ring pp_play_delay_ring_bytes bytes.  One launch. */
int pp_play_delay_push(const float* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width, int32_t depth,
                       const int32_t* delay, int32_t* age, float* ring, float* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
