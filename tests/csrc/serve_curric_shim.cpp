// serve_curric_shim.cpp — the serve-curriculum arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_serve_curric_device.h) compiled for
// the host and walked in the kernels' order, as serve_shim.cpp does for the serve plan.  TEST INFRASTRUCTURE ONLY.  Built by
// tests/serve_curric_shim_binding.py with -ffp-contract=off, the switch ppenv_serve_curric.hip is compiled with.  curric->cells and the
// state's pointers are host pointers here.
#include <cstddef>

#include "../../isaacgym_amd/csrc/ppenv_serve_curric_device.h"

extern "C" {

// sizeof(pp_serve_curric), its fields' offsets in declaration order, sizeof(pp_serve_curric_state), its fields' offsets
void curric_shim_layout(size_t* o) {
    const size_t v[] = {sizeof(pp_serve_curric), offsetof(pp_serve_curric, num_envs), offsetof(pp_serve_curric, env_id_offset), offsetof(pp_serve_curric, seed),
                        offsetof(pp_serve_curric, form), offsetof(pp_serve_curric, layout), offsetof(pp_serve_curric, reset_rows), offsetof(pp_serve_curric, num_agents),
                        offsetof(pp_serve_curric, bins), offsetof(pp_serve_curric, power), offsetof(pp_serve_curric, mix), offsetof(pp_serve_curric, alpha),
                        offsetof(pp_serve_curric, cells), sizeof(pp_serve_curric_state), offsetof(pp_serve_curric_state, count),
                        offsetof(pp_serve_curric_state, next_bin), offsetof(pp_serve_curric_state, cur_bin), offsetof(pp_serve_curric_state, ret),
                        offsetof(pp_serve_curric_state, games), offsetof(pp_serve_curric_state, mean), offsetof(pp_serve_curric_state, dropped),
                        offsetof(pp_serve_curric_state, cdf)};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) o[i] = v[i];
}

// the constants of the header: max bins, max power, the draw index, the fold's chunk
void curric_shim_consts(int64_t* o) { o[0] = PP_CURRIC_MAX_BINS; o[1] = PP_CURRIC_MAX_POWER; o[2] = PP_CURRIC_RNG_INDEX; o[3] = PP_CURRIC_FOLD_CHUNK; o[4] = PP_CURRIC_DROPPED; }

int curric_shim_invalid(const pp_serve_curric* c, const pp_serve_cell* cells) { return pp::curric_invalid(*c, cells); }

uint32_t curric_shim_u24(uint64_t seed, uint32_t gid, uint32_t j) { return pp::curric_u24(seed, gid, j); }
float curric_shim_uniform(uint64_t seed, uint32_t gid, uint32_t j) { return pp::rng_uniform(seed, gid, j, PP_CURRIC_RNG_INDEX); }
int32_t curric_shim_bin(const uint32_t* cdf, int32_t bins, uint32_t u24) { return pp::curric_bin_of(pp::CurricTable{cdf}, bins, u24); }
int64_t curric_shim_q(float x) { return pp::curric_q(x); }

// pp_serve_curric_fill on host memory: workgroup 0's table, then the envs
void curric_shim_fill(const pp_serve_curric* c, int32_t bins, const pp_serve_curric_state* s, float* out) {
    for (int32_t b = 0; b < bins; ++b) s->cdf[b] = pp::curric_uniform_cdf(bins, b);
    for (int32_t e = 0; e < c->num_envs; ++e) pp::curric_fill_env(*c, bins, e, *s, out);
}

// pp_serve_curric_step on host memory, env by env
void curric_shim_step(const pp_serve_curric* c, const float* rew, const int64_t* reset, const pp_serve_curric_state* s, float* out, int32_t* fin_bin_t,
                      int64_t* fin_q_t) {
    for (int32_t e = 0; e < c->num_envs; ++e) pp::curric_step_env(*c, e, rew, reset, *s, out, fin_bin_t, fin_q_t);
}

// pp_serve_curric_fold on host memory: a row per chunk of PP_CURRIC_FOLD_CHUNK entries, the rows added in chunk order
void curric_shim_fold(const int32_t* fin_bin, const int64_t* fin_q, int64_t count, int32_t bins, int64_t* tot) {
    for (int32_t k = 0; k < 3 * bins; ++k) tot[k] = 0;
    for (int64_t lo = 0; lo < count; lo += PP_CURRIC_FOLD_CHUNK) {
        int64_t row[3][PP_CURRIC_MAX_BINS] = {};
        const int64_t hi = lo + PP_CURRIC_FOLD_CHUNK < count ? lo + PP_CURRIC_FOLD_CHUNK : count;
        for (int64_t i = lo; i < hi; ++i) {
            const int kind = pp::curric_fold_kind(fin_bin[i], fin_q[i], bins);
            if (kind == 0) { row[0][fin_bin[i]] += 1; row[1][fin_bin[i]] += fin_q[i]; }
            if (kind == 2) row[2][fin_bin[i]] += 1;
        }
        for (int k = 0; k < 3; ++k)
            for (int32_t b = 0; b < bins; ++b) tot[(size_t)k * bins + b] += row[k][b];
    }
}

// pp_serve_curric_update on host memory: the four phases, each over all bins before the next (the kernel's barriers)
void curric_shim_update(const pp_serve_curric* c, int32_t bins, const int64_t* tot, const pp_serve_curric_state* s) {
    double w[PP_CURRIC_MAX_BINS], p[PP_CURRIC_MAX_BINS];
    for (int32_t b = 0; b < bins; ++b) pp::curric_ema_bin(*c, bins, b, tot, s->games, s->mean, s->dropped);
    for (int32_t b = 0; b < bins; ++b) w[b] = pp::curric_weight_bin(*c, bins, b, s->games, s->mean);
    for (int32_t b = 0; b < bins; ++b) p[b] = pp::curric_prob_bin(*c, bins, b, w);
    for (int32_t b = 0; b < bins; ++b) s->cdf[b] = pp::curric_cdf_bin(bins, b, p);
}

}
