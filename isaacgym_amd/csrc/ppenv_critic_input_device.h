// ppenv_critic_input_device.h — the per-element rules of the privileged critic inputs (include/ppenv_critic_input.h): the table's
// validation, where an element of a source lives, its conversion to float, and the normalise-and-clamp of one value.
//
// PP_HD like the other *_device.h headers: the kernels in ppenv_critic_input.hip and a host build compile this text.  The only
// arithmetic is prepare's (x - mean) * inv_std, clamped: two operations, each rounded on its own (the unit is built unfused).
#pragma once

#include <math.h>

#include "ppenv_device.h"
#include "../../include/ppenv_critic_input.h"

namespace pp {

enum { CRITIC_BLOCK = 256, CRITIC_TILE_ROWS = 64, CRITIC_TILE_COLS = 64 };

// 0 = valid; otherwise the index of upload's text, *which = the source it is about (-1: the table itself).  *total = P.
PP_HD int critic_table_invalid(const pp_critic_table& t, int32_t* which, int32_t* total) {
    *which = -1;
    *total = 0;
    if (t.num_agents != 1 && t.num_agents != 2) return 2;
    if (t.rows < 1 || t.rows % t.num_agents) return 1;
    if (t.sources < 1 || t.sources > PP_CRITIC_MAX_SOURCES) return 3;
    const int64_t envs = t.rows / t.num_agents;
    int64_t sum = 0;
    for (int32_t s = 0; s < t.sources; s++) {
        const pp_critic_source& c = t.source[s];
        *which = s;
        if (!c.p) return 4;
        if (c.kind != PP_CRITIC_F32 && c.kind != PP_CRITIC_I32) return 5;
        if (c.layout != PP_CRITIC_ROW_MAJOR && c.layout != PP_CRITIC_TABLE_MAJOR) return 6;
        if (c.cols < 1 || c.cols > PP_CRITIC_MAX_COLS) return 7;
        if (c.stride < (c.layout == PP_CRITIC_ROW_MAJOR ? (int64_t)c.cols : envs)) return 8;
        sum += c.cols;
    }
    *which = -1;
    if (sum > PP_CRITIC_MAX_COLS) return 9;
    *total = (int32_t)sum;
    return 0;
}

// element (r, c) of a source for actor row r, as the float the privileged row holds
PP_HD float critic_element(const pp_critic_source& s, int32_t num_agents, int64_t r, int32_t c) {
    const int64_t at = s.layout == PP_CRITIC_ROW_MAJOR ? r * s.stride + c : (int64_t)c * s.stride + r / num_agents;
    return s.kind == PP_CRITIC_I32 ? (float)((const int32_t*)s.p)[at] : ((const float*)s.p)[at];
}

// ppenv_mlp_prepare_input's value of one element, before the rounding to fp16
PP_HD float critic_normalise(float x, float mean, float inv_std, float clip) {
    return fminf(fmaxf((x - mean) * inv_std, -clip), clip);
}

}  // namespace pp
