// history_shim.cpp — the observation and action history of the HIP kernel (isaacgym_amd/csrc/ppenv_history_device.h) compiled for the host
// and walked in the kernel's order: workgroup by workgroup, first the rows' start words, then the 16-byte pieces.
// TEST INFRASTRUCTURE ONLY.  Built by tests/history_shim_binding.py.
#include "../../isaacgym_amd/csrc/ppenv_history_device.h"

extern "C" {

int32_t history_shim_width(int32_t n, int32_t A, int32_t Ho, int32_t Ha) { return pp::history_width(n, A, Ho, Ha); }

int32_t history_shim_rows_per_block(int32_t W) { return pp::history_rows_per_block(W); }

// pp::history_source of word c -> kind, col, left
void history_shim_source(int32_t n, int32_t A, int32_t Ho, int32_t Ha, int32_t start, int32_t c, int32_t* out) {
    const pp::history_shape s = {n, A, Ho, Ha, pp::history_width(n, A, Ho, Ha)};
    const pp::history_src o = pp::history_source(s, start != 0, c);
    out[0] = o.kind, out[1] = o.col, out[2] = o.left;
}

// pp_history_push on host memory (the arguments are taken as valid)
void history_shim_push(const uint32_t* obs, int64_t ld_obs, const uint32_t* act, int64_t ld_act, const int64_t* done, const uint32_t* prev, int64_t ld_prev,
                       uint32_t* next, int64_t ld_next, int32_t rows, int32_t num_agents, int32_t n, int32_t A, int32_t Ho, int32_t Ha, float lo, float hi) {
    const pp::history_shape s = {n, A, Ho, Ha, pp::history_width(n, A, Ho, Ha)};
    const int32_t per = pp::history_rows_per_block(s.W), pieces = pp::history_pieces(s.W);
    for (int64_t r0 = 0; r0 < rows; r0 += per) {                  // history_push_kernel, one workgroup
        const int32_t m = rows - r0 < per ? (int32_t)(rows - r0) : per;
        int32_t start_of[pp::HISTORY_BLOCK];
        for (int32_t t = 0; t < m; ++t) start_of[t] = pp::history_start(prev != nullptr, done, num_agents, r0 + t) ? 1 : 0;
        for (int32_t i = 0; i < m * pieces; ++i) {
            const int32_t row = i / pieces, p = i - row * pieces;
            const int64_t r = r0 + row;
            pp::history_move_piece(obs + r * ld_obs, act ? act + r * ld_act : nullptr, prev ? prev + r * ld_prev : nullptr, next + r * ld_next, s,
                                   start_of[row] != 0, p, lo, hi);
        }
    }
}

}
