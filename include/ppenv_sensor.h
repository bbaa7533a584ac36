/*
 * ppenv_sensor.h — C ABI of the SENSOR LINE: additive Gaussian noise and sample dropouts on the sensing path (the env's observations on
 * their way to the policy) and on the command path (the policy's actions on their way to the env), the noise-and-dropout sibling of the
 * delay lines (ppenv_play_delay.h, ppenv_train_delay.h).  A per-row amplitude, a per-column scale, a per-row dropout probability with
 * hold-last-sample; kept on the device and keyed by (seed, env, episode, step), so paired cells of a sweep see the same standard normals
 * (isaacgym_amd.sensor.SensorLine, play's obs_noise / obs_drop / action_noise / action_drop axes, RolloutCollector / PPOTrainer(obs_noise=,
 * obs_drop=, action_noise=, action_drop=)).  The step kernels and their two by-value amplitudes are not involved.
 *
 * THERE IS NO REFERENCE FOR THIS.  Like the delay lines', the rule below is this build's own specification: the project this one is
 * modelled on adds no such noise and drops no sample, so no oracle pins it; the tests check the kernel against the rule restated twice (a
 * host build of the device header, and numpy: isaacgym_amd.sensor.reference with scene.sensor_draws).
 *
 * A CHANNEL is `rows` actor rows (num_agents * num_envs, A = num_agents 1 or 2; env e owns rows A * e .. A * e + A - 1) of `width` W 32-bit
 * floats, 1 <= W <= PP_PLAY_DELAY_MAX_WIDTH.  Device tensors: sigma[rows] and drop[rows] (fp32: the row's noise amplitude and its dropout
 * probability), age[rows] and episode[rows] (int32: samples into the running episode, episodes begun), held[rows][W] (fp32: the values last
 * delivered), col_scale[W] (fp32, all >= 0: the column's share of the row's amplitude) and col_hold[W] (int32, 0 or 1: whether a dropout
 * holds the column).
 *
 * THE RULE.  One push per control step.  Per row r of env e = r / A, with the launch constants c (pp_sensor_consts):
 *
 *     a   = (done != NULL && done[A * e] != 0) ? 0 : age[r]          the delay lines' rule: all 64 bits of agent 0's word
 *     key = A * (c.env_id_offset + (c.key_period ? e % c.key_period : e)) + r % A                                       (uint32)
 *     if (a == 0) { n = episode[r];  episode[r] = n + 1              the first sample of an episode (also the first push after a reset)
 *                   if (c.draw) { sigma[r] = c.sigma_lo + (c.sigma_hi - c.sigma_lo) * U(LEVEL, key, n, 0)
 *                                 drop[r]  = c.drop_lo  + (c.drop_hi  - c.drop_lo ) * U(LEVEL, key, n, 1) } }
 *     else n = episode[r] - 1
 *     dropped = a > 0 && drop[r] > 0 && U(DROP, key, n, a) < drop[r]
 *     for column col, pair p = col >> 1, P = (W + 1) >> 1:
 *         s = sigma[r] * col_scale[col]                              one fp32 product
 *         if (s == 0) v = in[r][col]                                 a BITWISE copy: -0.0 and NaN payloads survive
 *         else { (g0, g1) = BoxMuller(U(NOISE, key, n, 2 * (a * P + p)), U(NOISE, key, n, 2 * (a * P + p) + 1))
 *                v = in[r][col] + s * (col & 1 ? g1 : g0) }          the product rounded, then the sum: no contraction
 *         if (col_hold[col]) { if (dropped) v = held[r][col]; else held[r][col] = v; }
 *         out[r][col] = v
 *     age[r] = a + 1
 *
 * U(part, key, n, k) is rng_uniform(s_part, key, n, k) of isaacgym_amd/csrc/ppenv_device.h (the counter RNG of every other draw here:
 * three rounds of hash32 keyed (seed, gid, episode, k), 24 bits to a float in [0, 1)), with
 * s_part = mix64(c.seed + 0x9E3779B97F4A7C15 * (1 + 3 * c.channel + part)) and part NOISE 0, DROP 1, LEVEL 2: the three families of draws
 * of the two channels never share a stream.  `seed` is a STREAM seed (isaacgym_amd.scene.stream_seed with STREAM_SENSOR).  The uniforms
 * and every integer are bit-exact between the device, a host build and numpy.  The level draws round the product, then the sum.
 *
 * BoxMuller(u1, u2) is dr_gauss_pair's arithmetic (ppenv_device.h) from two given uniforms: rad = sqrt(-2 ln max(u1, 2^-24)),
 * g0 = rad * cos(2 pi u2), g1 = rad * sin(2 pi u2) — on the device with the hardware's log2 / sqrt / cos / sin (which take the angle in
 * revolutions), on the host with libm.  The two differ by the transcendentals' error: at most 5.0e-7 of a unit normal, measured
 * (tests/test_rng_streams_gpu.py).  Both branches of a pair are used; a pair whose two s are zero draws nothing.
 *
 * WHAT FOLLOWS FROM THE RULE.
 *   - The first sample of an episode is never dropped (a > 0 is required), so held[r][:] is written at a == 0 before it can be read:
 *     nothing is carried across a reset, and `held` is never cleared.
 *   - A dropped sample delivers the values last DELIVERED, with their noise: the receiver sees a frozen frame, not a clean one.
 *   - A row with sigma = 0 and drop = 0 is a bitwise copy of its input.
 *   - With draw == 0 the kernel never writes sigma[] / drop[]: they are the caller's table (play: one value per sweep cell).  With
 *     draw == 1 they are device state like the training delay line's delay[], redrawn at every episode start (training).
 *   - The key is the GLOBAL row: two shards with the right env_id_offset reproduce one handle, bit for bit.
 *   - With key_period set, env e and env e + key_period see the same uniforms (common random numbers across the paired cells of a sweep):
 *     their standard normals are equal, and their s * g scale with sigma.
 *
 * One launch per push, of the delay lines' shape: a workgroup owns pp::delay_rows_per_block(W) whole rows; one lane per row does the
 * bookkeeping (age, episode, the two level draws, the drop decision) and leaves it in LDS; after a barrier all lanes walk the rows' COLUMN
 * PAIRS, consecutive lanes on consecutive pairs.  A pair moves as one 8-byte access where source and destination (and `held`, where both
 * columns hold) are 8-byte aligned, word by word otherwise and at an odd W's last column: row starts are only 4-byte aligned in general.
 * `held` is touched only for col_hold columns.  No atomics, no host-side counter, no word read by one workgroup and written by another:
 * a captured launch replays like an eager one.  `out` is the caller's pointer with its own stride (a slice of a horizon buffer: no copy).
 * The row's arithmetic is isaacgym_amd/csrc/ppenv_sensor_device.h, which the tests also compile for the host.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation; returns 0 or a negative PPENV_E* code (ppenv.h) with the message in
 * ppenv_last_error().  Refused with PPENV_EINVAL before any device call: everything pp_train_delay_push refuses (a NULL pointer, `done`
 * excepted; rows < 1 or no multiple of num_agents; num_agents not 1 or 2; width outside 1..PP_PLAY_DELAY_MAX_WIDTH; a stride below width;
 * a NULL constants struct), a NULL table, a negative or non-finite sigma_lo / sigma_hi, drop_lo / drop_hi outside [0, 1], lo > hi,
 * key_period < 0, env_id_offset < 0, channel not 0 or 1, draw not 0 or 1.
 */
#ifndef PPENV_SENSOR_H
#define PPENV_SENSOR_H

#include "ppenv_play_delay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_SENSOR_COMMAND 0                           /* channel: the policy's actions on their way to the env */
#define PP_SENSOR_SENSING 1                           /* channel: the env's observations on their way to the policy */
#define PP_SENSOR_NOISE 0                             /* part: the Box-Muller uniforms of a column pair */
#define PP_SENSOR_DROP 1                              /* part: the drop decision of a row's sample */
#define PP_SENSOR_LEVEL 2                             /* part: the per-episode amplitude and dropout probability */

/* The launch constants of a line: read on the host, passed to the kernel by value. */
typedef struct pp_sensor_consts {
    float sigma_lo, sigma_hi;                         /* the amplitude's range, 0 <= lo <= hi, finite (read only where draw == 1) */
    float drop_lo, drop_hi;                           /* the dropout probability's range, 0 <= lo <= hi <= 1 (read only where draw == 1) */
    int32_t draw;                                     /* 0: sigma[] / drop[] are the caller's table; 1: the kernel draws them per episode */
    uint64_t seed;                                    /* a STREAM seed */
    int32_t env_id_offset;                            /* the global id of env 0 (a data-parallel rank's shard) */
    int32_t key_period;                              /* 0, or the envs per paired cell: env e is keyed as env e % key_period */
    int32_t channel;                                  /* PP_SENSOR_COMMAND or PP_SENSOR_SENSING */
} pp_sensor_consts;

/* Bytes of each of sigma / drop / age / episode (4 * rows) and of `held` (4 * rows * width); 0 for sizes the entries refuse. */
size_t pp_sensor_table_bytes(int32_t rows);
size_t pp_sensor_held_bytes(int32_t rows, int32_t width);

/* age[0 .. rows) and episode[0 .. rows) to zero.  One launch.  sigma, drop and held are left as they are. */
int pp_sensor_reset(int32_t rows, int32_t* age, int32_t* episode, void* stream);

/* One control step.  in [rows, ld_in] and out [rows, ld_out]: fp32, strides in ELEMENTS, `in` is not modified and must not overlap out
 * or held; done [rows] int64 or NULL; col_scale [width] fp32; col_hold [width] int32; sigma, drop [rows] fp32; age, episode [rows] int32;
 * held [rows, width] fp32.  One launch. */
int pp_sensor_push(const float* in, int64_t ld_in, const int64_t* done, int32_t rows, int32_t num_agents, int32_t width,
                   const pp_sensor_consts* consts, const float* col_scale, const int32_t* col_hold, float* sigma, float* drop, int32_t* age,
                   int32_t* episode, float* held, float* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
