// adr_shim.cpp — the ADR arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_dr_adr_device.h) compiled for the host and walked in the
// kernels' order, as serve_curric_shim.cpp does for the serve curriculum.  TEST INFRASTRUCTURE ONLY.  Built by tests/adr_shim_binding.py
// with -ffp-contract=off, the switch ppenv_dr_adr.hip is compiled with.  The dims' tables and the state's pointers are host pointers here.
#include <cstddef>

#include "../../isaacgym_amd/csrc/ppenv_dr_adr_device.h"

extern "C" {

// sizeof(pp_dr_adr_dim), its fields' offsets in declaration order; the same for pp_dr_adr and pp_dr_adr_state
void adr_shim_layout(size_t* o) {
    const size_t v[] = {sizeof(pp_dr_adr_dim), offsetof(pp_dr_adr_dim, table), offsetof(pp_dr_adr_dim, rows), offsetof(pp_dr_adr_dim, start_lo),
                        offsetof(pp_dr_adr_dim, start_hi), offsetof(pp_dr_adr_dim, limit_lo), offsetof(pp_dr_adr_dim, limit_hi), offsetof(pp_dr_adr_dim, step),
                        sizeof(pp_dr_adr), offsetof(pp_dr_adr, num_envs), offsetof(pp_dr_adr, env_id_offset), offsetof(pp_dr_adr, seed),
                        offsetof(pp_dr_adr, reset_rows), offsetof(pp_dr_adr, num_agents), offsetof(pp_dr_adr, dims), offsetof(pp_dr_adr, thr),
                        offsetof(pp_dr_adr, min_games), offsetof(pp_dr_adr, t_low), offsetof(pp_dr_adr, t_high), offsetof(pp_dr_adr, reserved),
                        offsetof(pp_dr_adr, dim), sizeof(pp_dr_adr_state), offsetof(pp_dr_adr_state, range), offsetof(pp_dr_adr_state, draws),
                        offsetof(pp_dr_adr_state, slot), offsetof(pp_dr_adr_state, ret), offsetof(pp_dr_adr_state, acc_n), offsetof(pp_dr_adr_state, acc_q),
                        offsetof(pp_dr_adr_state, games), offsetof(pp_dr_adr_state, dropped), offsetof(pp_dr_adr_state, mean),
                        offsetof(pp_dr_adr_state, widened), offsetof(pp_dr_adr_state, narrowed)};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) o[i] = v[i];
}

// the constants of the header: the coin's and the pick's draw index, the most slots, the tables' and the rows' limits
void adr_shim_consts(int64_t* o) { o[0] = PP_ADR_COIN_INDEX; o[1] = PP_ADR_PICK_INDEX; o[2] = PP_ADR_MAX_SLOTS; o[3] = PPENV_DR_MAX_TABLES; o[4] = PPENV_DR_MAX_ROWS; }

int adr_shim_invalid(const pp_dr_adr* a, double boundary_frac, int32_t* which) { return pp::adr_invalid(*a, boundary_frac, which); }
uint32_t adr_shim_thr(double boundary_frac) { return pp::adr_thr(boundary_frac); }
uint32_t adr_shim_u24(uint64_t sd, uint32_t gid, uint32_t j, uint32_t k) { return pp::adr_u24(sd, gid, j, k); }
float adr_shim_uniform(uint64_t sd, uint32_t gid, uint32_t j, uint32_t k) { return pp::rng_uniform(sd, gid, j, k); }
int32_t adr_shim_slot(uint64_t seed, uint32_t gid, uint32_t j, uint32_t thr, int32_t dims) { return pp::adr_slot_of(seed, gid, j, thr, dims); }

// pp_dr_adr_fill on host memory: workgroup 0's ranges, then the envs
void adr_shim_fill(const pp_dr_adr* a, int32_t dims, const pp_dr_adr_state* s) {
    for (int32_t k = 0; k < 2 * dims; ++k) s->range[k] = pp::AdrStarts{}(*a, k >> 1, k & 1);
    for (int32_t e = 0; e < a->num_envs; ++e) pp::adr_fill_env(*a, dims, e, *s);
}

// pp_dr_adr_step on host memory, env by env
void adr_shim_step(const pp_dr_adr* a, const float* rew, const int64_t* reset, const pp_dr_adr_state* s, int32_t* fin_slot_t, int64_t* fin_q_t) {
    for (int32_t e = 0; e < a->num_envs; ++e) pp::adr_step_env(*a, e, rew, reset, *s, fin_slot_t, fin_q_t);
}

// pp_dr_adr_update on host memory, slot by slot
void adr_shim_update(const pp_dr_adr* a, int32_t dims, const int64_t* tot, const pp_dr_adr_state* s) {
    for (int32_t k = 0; k < 2 * dims + 1; ++k) pp::adr_update_slot(*a, dims, k, tot, *s);
}

}
