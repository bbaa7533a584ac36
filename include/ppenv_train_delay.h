/*
 * ppenv_train_delay.h — C ABI of the CONTROL-LATENCY delay line of TRAINING: ppenv_play_delay.h's per-row ring, with the row's delay
 * DRAWN ON THE DEVICE at every episode start from a range lo .. hi of whole control steps (lo == hi: a fixed delay), one line for the
 * command path and one for the sensing path (isaacgym_amd.latency.DelayLine, RolloutCollector(action_delay=, obs_delay=),
 * PPOTrainer(action_delay=, obs_delay=), python -m isaacgym_amd.ppo --action-delay / --obs-delay).
 *
 * THERE IS NO REFERENCE FOR THIS.  Like ppenv_play_delay.h's, the rule below is this build's own specification: nothing in the project
 * this one is modelled on delays a command or an observation, so no oracle pins it; the tests check the kernel against the rule restated
 * twice (a host build of the device header, and numpy with scene.latency_draws).
 *
 * A CHANNEL is play's: `rows` actor rows (num_agents * num_envs; env e owns rows A * e .. A * e + A - 1) of `width` W 32-bit values, a ring
 * [K][rows][W], age[rows] and delay[rows] (int32) — and episode[rows] (int32), the number of episodes the row has begun.  K = hi + 1.
 * Here delay[] is DEVICE STATE WRITTEN BY THE KERNEL, not a table the host uploads.
 *
 * THE RULE.  One push per control step.  Per row r of env e = r / A, with the launch constants c (pp_train_delay_consts):
 *
 *     a = (done != NULL && done[A * e] != 0) ? 0 : age[r]            exactly pp::delay_index's rule: all 64 bits of agent 0's word
 *     if (a == 0) {                                                  the first sample of an episode (also the first push after a reset)
 *         n = episode[r];  episode[r] = n + 1
 *         d = c.lo + draw(c.seed, c.env_id_offset + e, n, c.channel, c.hi - c.lo + 1);  delay[r] = d
 *     } else d = delay[r]
 *     ring[a % K][r][:] = in[r][:];  s = a - min(a, d);  out[r][:] = ring[s % K][r][:];  age[r] = a + 1        ppenv_play_delay.h, unchanged
 *
 * THE DRAW.  draw(seed, gid, n, k, span) is the hash32 chain of rng_uniform (isaacgym_amd/csrc/ppenv_device.h) keyed (seed, gid,
 * episode = n, k), reduced in integer arithmetic only: h = hash32(gid ^ low32(seed)); h = hash32(h + n * 0x9E3779B9 + high32(seed));
 * h = hash32(h + (k + 1) * 0x85EBCA6B); draw = ((uint64_t)(h >> 8) * span) >> 24, a value in 0 .. span - 1.  No floating point: a host
 * build and the device agree bit for bit, and span == 1 gives 0 for every key.  `seed` is a STREAM seed (isaacgym_amd.scene.stream_seed
 * with STREAM_LATENCY).  The key is the ENV, so both rows of a 4-actor env hold the same delay; the two channels differ in k.
 * isaacgym_amd.scene.latency_draws restates it in numpy.
 *
 * A delay changes only where a == 0, where the slot read IS the slot written, so play's invariant holds as it stands: no slot is read
 * before it was written in the running episode (s <= a, a - s <= d <= hi < K), and the ring is never cleared.
 *
 * One launch per push, of play's shape: a workgroup owns pp::delay_rows_per_block(W) whole rows; one lane per row does the bookkeeping
 * (age, episode, the draw, delay) and leaves the two slots in LDS; after a barrier all lanes walk the rows' words, consecutive lanes on
 * consecutive words.  No atomics, no host-side counter, no word read by one workgroup and written by another: a captured launch replays
 * like an eager one.  `out` is the caller's pointer with its own stride (a slice of a horizon buffer: no copy).  The row's bookkeeping is
 * isaacgym_amd/csrc/ppenv_train_delay_device.h, which the tests also compile for the host; the index and move functions are
 * ppenv_play_delay_device.h's, by inclusion.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the message in
 * ppenv_last_error().  Refused with PPENV_EINVAL before any device call: everything pp_play_delay_push refuses (a NULL pointer, `done`
 * excepted; rows < 1 or no multiple of num_agents; num_agents not 1 or 2; width outside 1..PP_PLAY_DELAY_MAX_WIDTH; a stride below width),
 * a NULL constants struct, lo < 0, lo > hi, hi > PP_PLAY_DELAY_MAX, channel not 0 or 1.
 */
#ifndef PPENV_TRAIN_DELAY_H
#define PPENV_TRAIN_DELAY_H

#include "ppenv_play_delay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_TRAIN_DELAY_COMMAND 0                      /* channel: the policy's actions on their way to the env */
#define PP_TRAIN_DELAY_SENSING 1                      /* channel: the env's observations on their way to the policy */

/* The launch constants of a line: read on the host, passed to the kernel by value. */
typedef struct pp_train_delay_consts {
    int32_t lo, hi;                                   /* the delay's range in control steps, 0 <= lo <= hi <= PP_PLAY_DELAY_MAX; the ring has hi + 1 slots */
    uint64_t seed;                                    /* a STREAM seed */
    int32_t env_id_offset;                            /* the global id of env 0 (a data-parallel rank's shard) */
    int32_t channel;                                  /* PP_TRAIN_DELAY_COMMAND or PP_TRAIN_DELAY_SENSING */
} pp_train_delay_consts;

/* Bytes of `ring` (4 * (hi + 1) * rows * width) and of each of age / delay / episode (4 * rows); 0 for sizes the entries refuse. */
size_t pp_train_delay_ring_bytes(int32_t rows, int32_t width, int32_t hi);
size_t pp_train_delay_table_bytes(int32_t rows);

/* age[0 .. rows) and episode[0 .. rows) to zero.  One launch.  The ring and delay[] are left as they are. */
int pp_train_delay_reset(int32_t rows, int32_t* age, int32_t* episode, void* stream);

/* One control step.  in [rows, ld_in] and out [rows, ld_out]: 32-bit values, strides in ELEMENTS, `in` is not modified and must not
 * overlap out or ring; done [rows] int64 or NULL; delay, age, episode [rows] int32; ring pp_train_delay_ring_bytes bytes.  One launch. */
int pp_train_delay_push(const float* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width,
                        const pp_train_delay_consts* consts, int32_t* delay, int32_t* age, int32_t* episode, float* ring, float* out, int64_t ld_out,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif
