// ppenv_history_device.h — the per-row column map of the observation and action history (include/ppenv_history.h): which word of obs, act
// or the previous wide row a word of the next wide row comes from, the start test of a row, and the move of one 16-byte piece of `next`.
//
// PP_HD like the delay lines' device headers: the HIP kernel in ppenv_history.hip and the tests' host build (tests/csrc/history_shim.cpp,
// g++) compile this text, and the two must agree BYTE FOR BYTE.  Words are moved as uint32_t; the only arithmetic is the clamp of a_1,
// fminf(fmaxf(x, lo), hi), which a NaN leaves as lo.
#pragma once

#include <math.h>

#include "ppenv_device.h"
#include "../../include/ppenv_history.h"

namespace pp {

// the rows a workgroup of the push kernel owns: about four 16-byte pieces per lane, whole rows, at most one row per lane
enum { HISTORY_BLOCK = 256, HISTORY_PIECES = 4 * HISTORY_BLOCK };
enum { HISTORY_OBS = 0, HISTORY_PREV = 1, HISTORY_ACT = 2, HISTORY_ZERO = 3 };

struct history_shape {
    int32_t n, A, Ho, Ha, W;
};

// W, or 0 for a history the push refuses
PP_HD int32_t history_width(int32_t n, int32_t A, int32_t Ho, int32_t Ha) {
    if (n < 1 || A < 1 || Ho < 0 || Ho > PP_HISTORY_MAX || Ha < 0 || Ha > PP_HISTORY_MAX || (Ho == 0 && Ha == 0)) return 0;
    const int64_t w = (int64_t)(Ho + 1) * n + (int64_t)Ha * A;
    return w > PP_HISTORY_MAX_WIDTH ? 0 : (int32_t)w;
}

// 16-byte pieces of `next` a row can touch: its W words begin at any of the four word phases of a piece
PP_HD int32_t history_pieces(int32_t W) { return (W + 3) / 4 + 1; }

PP_HD int32_t history_rows_per_block(int32_t W) {
    const int32_t r = HISTORY_PIECES / history_pieces(W);
    return r < 1 ? 1 : r > HISTORY_BLOCK ? HISTORY_BLOCK : r;
}

// row r starts a history: there is no previous row, or agent 0 of its env has a done word that is not zero (all 64 bits: pp::delay_index's rule)
PP_HD bool history_start(bool have_prev, const int64_t* done, int32_t num_agents, int64_t r) {
    return !have_prev || (done != nullptr && done[(size_t)num_agents * (size_t)(r / num_agents)] != 0);
}

struct history_src {
    int32_t kind;                                                // HISTORY_*
    int32_t col;                                                 // the word of that source's row
    int32_t left;                                                // words from here to the end of the run: c + i comes from col + i for i < left
};

// where word c (0 <= c < W) of the next wide row comes from
PP_HD history_src history_source(const history_shape& s, bool start, int32_t c) {
    const int32_t obs_end = (s.Ho + 1) * s.n;
    history_src o;
    if (c < s.n) {                                               // o_0: the new observation
        o.kind = HISTORY_OBS, o.col = c, o.left = s.n - c;
    } else if (c < obs_end) {
        if (start) {                                             // o_k: the first sample held
            o.kind = HISTORY_OBS, o.col = c % s.n, o.left = s.n - o.col;
        } else {                                                 // o_k = prev.o_{k-1}: the observation slots move up by one
            o.kind = HISTORY_PREV, o.col = c - s.n, o.left = obs_end - c;
        }
    } else if (start) {                                          // a_j = 0
        o.kind = HISTORY_ZERO, o.col = 0, o.left = s.W - c;
    } else if (c < obs_end + s.A) {                              // a_1: the action issued on prev
        o.kind = HISTORY_ACT, o.col = c - obs_end, o.left = obs_end + s.A - c;
    } else {                                                     // a_j = prev.a_{j-1}
        o.kind = HISTORY_PREV, o.col = c - s.A, o.left = s.W - c;
    }
    return o;
}

PP_HD uint32_t history_clamp(uint32_t w, float lo, float hi) {
    float x;
    memcpy(&x, &w, 4);
    x = fminf(fmaxf(x, lo), hi);
    memcpy(&w, &x, 4);
    return w;
}

struct alignas(16) history_w4 {
    uint32_t w[4];
};

PP_HD const uint32_t* history_row_of(int32_t kind, const uint32_t* obs_r, const uint32_t* act_r, const uint32_t* prev_r) {
    return kind == HISTORY_OBS ? obs_r : kind == HISTORY_ACT ? act_r : prev_r;
}

// Piece p of a row whose four pointers are the row's first words (act_r, prev_r: never read where they are NULL, by history_source's
// kinds).  Piece p is the p-th 16-byte word of memory the row of `next` touches: its words 4 p - phase .. 4 p - phase + 3, cut to 0 .. W.
// A whole piece inside one run whose source is 16-byte aligned as well moves as one 16-byte word, everything else word by word.
PP_HD void history_move_piece(const uint32_t* obs_r, const uint32_t* act_r, const uint32_t* prev_r, uint32_t* next_r, const history_shape& s, bool start,
                              int32_t p, float lo, float hi) {
    const int32_t phase = (int32_t)(((uintptr_t)next_r >> 2) & 3u);
    const int32_t c0 = 4 * p - phase;
    if (c0 >= s.W) return;
    if (c0 >= 0 && c0 + 4 <= s.W) {
        const history_src a = history_source(s, start, c0);
        if (a.left >= 4) {
            history_w4 v;
            if (a.kind == HISTORY_ZERO) {
                v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0u;
                *reinterpret_cast<history_w4*>(next_r + c0) = v;
                return;
            }
            const uint32_t* src = history_row_of(a.kind, obs_r, act_r, prev_r) + a.col;
            if (((uintptr_t)src & 15u) == 0) {
                v = *reinterpret_cast<const history_w4*>(src);
                if (a.kind == HISTORY_ACT)
                    for (int q = 0; q < 4; q++) v.w[q] = history_clamp(v.w[q], lo, hi);
                *reinterpret_cast<history_w4*>(next_r + c0) = v;
                return;
            }
        }
    }
    for (int q = 0; q < 4; q++) {
        const int32_t c = c0 + q;
        if (c < 0 || c >= s.W) continue;
        const history_src a = history_source(s, start, c);
        uint32_t w = 0u;
        if (a.kind != HISTORY_ZERO) {
            w = history_row_of(a.kind, obs_r, act_r, prev_r)[a.col];
            if (a.kind == HISTORY_ACT) w = history_clamp(w, lo, hi);
        }
        next_r[c] = w;
    }
}

}  // namespace pp
