// ppenv_sensor_device.h — the sensor line's arithmetic (include/ppenv_sensor.h): the three stream seeds of a channel, the counter RNG's
// uniforms, Box-Muller from two given uniforms, a row's bookkeeping for one push (age, episode, the two level draws, the drop decision)
// and the move of one column pair.  The launch shape (pp::delay_rows_per_block) is ppenv_play_delay_device.h's, by inclusion.
//
// PP_HD like the delay lines' device headers: the HIP kernel in ppenv_sensor.hip and the tests' host build (tests/csrc/sensor_shim.cpp, g++)
// compile this text.  The integers, the uniforms, the level draws, the drop decisions and every column whose s is zero agree BYTE FOR BYTE
// between the two; a noised value differs by the error of Box-Muller's transcendentals (hardware on the device, libm on the host) times s.
// Both builds take -ffp-contract=off -fsigned-zeros -fno-finite-math-only: s * g is rounded before it is added, and a zero row copies bits.
#pragma once

#include <math.h>
#include <string.h>

#include "ppenv_play_delay_device.h"
#include "../../include/ppenv_sensor.h"

namespace pp {

// NaN fails every comparison, +inf fails hi <= top
PP_HD bool sensor_range_ok(float lo, float hi, float top) { return lo >= 0.0f && lo <= hi && hi <= top; }

PP_HD bool sensor_consts_ok(const pp_sensor_consts& c) {
    return sensor_range_ok(c.sigma_lo, c.sigma_hi, 3.4028234664e38f) && sensor_range_ok(c.drop_lo, c.drop_hi, 1.0f) && (c.draw == 0 || c.draw == 1) &&
           c.key_period >= 0 && c.env_id_offset >= 0 && (c.channel == PP_SENSOR_COMMAND || c.channel == PP_SENSOR_SENSING);
}

PP_HD size_t sensor_held_bytes(int32_t rows, int32_t width) { return delay_ring_bytes(rows, width, 1); }

// s_part of the header: one stream seed per family of draws and channel.  Formed once per launch on the host.
struct sensor_seeds {
    uint64_t noise, drop, level;
};

PP_HD uint64_t sensor_part_seed(uint64_t seed, int32_t channel, int32_t part) {
    return mix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(1 + 3 * channel + part));
}

PP_HD sensor_seeds sensor_seeds_of(const pp_sensor_consts& c) {
    sensor_seeds s;
    s.noise = sensor_part_seed(c.seed, c.channel, PP_SENSOR_NOISE);
    s.drop = sensor_part_seed(c.seed, c.channel, PP_SENSOR_DROP);
    s.level = sensor_part_seed(c.seed, c.channel, PP_SENSOR_LEVEL);
    return s;
}

// rng_uniform(sd, key, n, k) (ppenv_device.h) in two halves: the two rounds of its hash chain that depend on the row alone, formed once per
// row, and the round that takes k.  sensor_uniform(sensor_chain(sd, key, n), k) == rng_uniform(sd, key, n, k), bit for bit.
PP_HD uint32_t sensor_chain(uint64_t sd, uint32_t key, uint32_t n) {
    const uint32_t h = hash32(key ^ (uint32_t)sd);
    return hash32(h + n * 0x9E3779B9u + (uint32_t)(sd >> 32));
}

PP_HD float sensor_uniform(uint32_t chain, uint32_t k) {
    return (float)(hash32(chain + (k + 1u) * 0x85EBCA6Bu) >> 8) * (1.0f / 16777216.0f);
}

// dr_gauss_pair's arithmetic (ppenv_device.h) from two given uniforms: the hardware's log2 / sqrt / cos / sin on the device (the angle in
// revolutions: exactly Box-Muller's 2 pi u2), libm on the host.
PP_HD void sensor_box_muller(float u1, float u2, float& g_cos, float& g_sin) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float rad = __builtin_amdgcn_sqrtf(-1.3862944f * __builtin_amdgcn_logf(fmaxf(u1, 5.9604645e-8f)));     // sqrt(-2 ln u1) = sqrt(-2 ln 2 log2 u1)
    g_cos = rad * __builtin_amdgcn_cosf(u2);
    g_sin = rad * __builtin_amdgcn_sinf(u2);
#else
    const float rad = sqrtf(-2.0f * logf(fmaxf(u1, 5.9604645e-8f)));
    g_cos = rad * cosf(6.2831853f * u2);
    g_sin = rad * sinf(6.2831853f * u2);
#endif
}

// what the bookkeeping lane of a row leaves for the lanes that walk the row's pairs
struct sensor_row {
    uint32_t chain;                                              // sensor_chain(NOISE seed, key, n)
    uint32_t base;                                               // a * P: pair p draws the uniforms 2 * (base + p) and 2 * (base + p) + 1
    float sigma;                                                 // sigma[r] of the running episode
    int32_t dropped;                                             // this sample is dropped: hold columns deliver `held`
};

// Row r's push: the only read and write of age[r] and episode[r]; where this sample is the first of an episode and c.draw is set, the only
// write of sigma[r] and drop[r].  The row's four words are read up front, as pp::train_delay_row reads its three: read only where needed,
// each would be another trip to memory on the one lane per row the workgroup's barrier waits for.
PP_HD sensor_row sensor_book(const int64_t* done, int32_t num_agents, int64_t r, int32_t width, const pp_sensor_consts& c, const sensor_seeds& sd, float* sigma,
                             float* drop, int32_t* age, int32_t* episode) {
    const int32_t age_r = age[r];
    const uint32_t ep = (uint32_t)episode[r];
    float sg = sigma[r], dp = drop[r];
    const uint32_t A = (uint32_t)num_agents, env = (uint32_t)r / A, agent = (uint32_t)r - env * A;      // r < rows <= 2^31 - 1: 32-bit divisions
    const int32_t a = (done != nullptr && done[(size_t)A * (size_t)env] != 0) ? 0 : age_r;             // all 64 bits of agent 0's word
    const uint32_t key = A * ((uint32_t)c.env_id_offset + (c.key_period ? env % (uint32_t)c.key_period : env)) + agent;
    const uint32_t n = a == 0 ? ep : ep - 1u;
    if (a == 0) {                                                // the first sample of an episode
        episode[r] = (int32_t)(ep + 1u);
        if (c.draw) {
            const uint32_t level = sensor_chain(sd.level, key, n);
            const float ws = (c.sigma_hi - c.sigma_lo) * sensor_uniform(level, 0u), wd = (c.drop_hi - c.drop_lo) * sensor_uniform(level, 1u);
            sg = c.sigma_lo + ws;                                // the product rounded, then the sum
            dp = c.drop_lo + wd;
            sigma[r] = sg;
            drop[r] = dp;
        }
    }
    age[r] = (int32_t)((uint32_t)a + 1u);
    sensor_row o;
    o.chain = sensor_chain(sd.noise, key, n);
    o.base = (uint32_t)a * (uint32_t)((width + 1) >> 1);
    o.sigma = sg;
    o.dropped = (a > 0 && dp > 0.0f && sensor_uniform(sensor_chain(sd.drop, key, n), (uint32_t)a) < dp) ? 1 : 0;
    return o;
}

// in + s * g on the bits of a float; s == 0: the word as it is (a negative zero and a NaN's payload survive)
PP_HD uint32_t sensor_value(uint32_t w, float s, float g) {
    if (s == 0.0f) return w;
    float x;
    memcpy(&x, &w, 4);
    const float sg = s * g;
    x = x + sg;
    memcpy(&w, &x, 4);
    return w;
}

struct alignas(8) sensor_w2 {
    uint32_t w[2];
};

PP_HD bool sensor_aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

// Pair p (columns 2 p and 2 p + 1, the second one missing at an odd W's end) of a row whose three pointers are the row's first words.
// The pair moves as one 8-byte access where `in_r + 2 p` and `out_r + 2 p` are both 8-byte aligned, word by word otherwise; `held` is
// touched only for col_hold columns, as one 8-byte access where both columns hold and it is aligned.
PP_HD void sensor_move_pair(const uint32_t* in_r, uint32_t* held_r, uint32_t* out_r, const float* col_scale, const int32_t* col_hold, int32_t width, int32_t p,
                            const sensor_row& row) {
    const int32_t c0 = 2 * p;
    const bool two = c0 + 1 < width;
    const float s0 = row.sigma * col_scale[c0], s1 = two ? row.sigma * col_scale[c0 + 1] : 0.0f;
    const bool h0 = col_hold[c0] != 0, h1 = two && col_hold[c0 + 1] != 0;
    float g0 = 0.0f, g1 = 0.0f;
    if (!(s0 == 0.0f && s1 == 0.0f)) {
        const uint32_t k = 2u * (row.base + (uint32_t)p);
        sensor_box_muller(sensor_uniform(row.chain, k), sensor_uniform(row.chain, k + 1u), g0, g1);
    }
    const bool wide = two && sensor_aligned8(in_r + c0) && sensor_aligned8(out_r + c0);
    uint32_t w0, w1 = 0u;
    if (wide) {
        const sensor_w2 v = *reinterpret_cast<const sensor_w2*>(in_r + c0);
        w0 = v.w[0], w1 = v.w[1];
    } else {
        w0 = in_r[c0];
        if (two) w1 = in_r[c0 + 1];
    }
    w0 = sensor_value(w0, s0, g0);
    w1 = sensor_value(w1, s1, g1);
    if (h0 && h1 && sensor_aligned8(held_r + c0)) {
        sensor_w2* h = reinterpret_cast<sensor_w2*>(held_r + c0);
        if (row.dropped) {
            const sensor_w2 v = *h;
            w0 = v.w[0], w1 = v.w[1];
        } else {
            sensor_w2 v;
            v.w[0] = w0, v.w[1] = w1;
            *h = v;
        }
    } else {
        if (h0) {
            if (row.dropped) w0 = held_r[c0];
            else held_r[c0] = w0;
        }
        if (h1) {
            if (row.dropped) w1 = held_r[c0 + 1];
            else held_r[c0 + 1] = w1;
        }
    }
    if (wide) {
        sensor_w2 v;
        v.w[0] = w0, v.w[1] = w1;
        *reinterpret_cast<sensor_w2*>(out_r + c0) = v;
    } else {
        out_r[c0] = w0;
        if (two) out_r[c0 + 1] = w1;
    }
}

}  // namespace pp
