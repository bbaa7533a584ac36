// play_act_sanitize_main.cpp — a stand-alone driver of play_act_shim.cpp (the actuator accounting's kernel bodies on the host) over one
// case per input layout, for a build under -fsanitize=address,undefined: every buffer is sized exactly as the C ABI says
// (include/ppenv_play_act.h), so an index past a plane, a partial or a struct is reported.  TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_play_act_host.py, never loaded into Python.  Prints the games of every group and exits 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "play_act_shim.cpp"

namespace {

uint32_t rng_state = 12345u;
float uniform() {                                              // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

// S envs per group, G groups, D dofs, A agents; aos: dof_states [N, D, 2] + dof_force [N, D], else [D][N] planes.
int run(int32_t S, int32_t G, int32_t D, int32_t A, bool aos, bool with_action, int steps, int64_t games_num) {
    const int64_t N = (int64_t)S * G;
    const int32_t parts = (S + PPENV_PLAY_BLOCK - 1) / PPENV_PLAY_BLOCK;
    std::vector<uint32_t> state((size_t)(1 + PP_PLAY_ACT_FIELDS * D) * N, 0x55555555u);
    std::vector<pp_play_act_group> group(G);
    std::vector<pp_play_act_joint> joint((size_t)G * D);
    std::vector<unsigned char> partial((size_t)G * parts * (sizeof(pp_play_act_group) + (size_t)D * sizeof(pp_play_act_joint)));
    std::vector<pp_play_act_limit> limits(D);
    for (int32_t d = 0; d < D; ++d) limits[d] = {-1.0f - 0.1f * d, 1.0f + 0.05f * d, 25.0f + d, 37.0f - 0.5f * d};
    const pp_play_act_thresholds thr = {0.98f, 0.98f, 0.02f, 1.0f};
    std::vector<float> states((size_t)N * D * 2), force((size_t)N * D), action((size_t)N * D);
    std::vector<int64_t> done((size_t)N * A);
    pp_play_act_inputs in;
    if (aos) {
        in.q = {states.data(), 2 * (int64_t)D, 2};
        in.qd = {states.data() + 1, 2 * (int64_t)D, 2};
        in.tau = {force.data(), D, 1};
    } else {
        in.q = {states.data(), 1, N};
        in.qd = {states.data() + (size_t)N * D, 1, N};
        in.tau = {force.data(), 1, N};
    }
    in.action = {with_action ? action.data() : nullptr, D, 1};
    play_act_shim_reset(S, G, D, state.data(), group.data(), joint.data());
    for (int s = 0; s < steps; ++s) {
        for (float& v : states) v = 80.0f * uniform() - 40.0f;
        for (float& v : force) v = 60.0f * uniform() - 30.0f;
        for (float& v : action) v = 3.0f * uniform() - 1.5f;
        for (int64_t e = 0; e < N; ++e) {
            const int64_t word = uniform() < 0.1f ? ((e & 1) ? 2 : (int64_t)1 << 32) : 0;
            for (int32_t a = 0; a < A; ++a) done[(size_t)A * e + a] = word;
        }
        play_act_shim_accumulate(&in, done.data(), S, G, A, D, games_num, limits.data(), &thr, state.data(), group.data(), joint.data(), partial.data());
    }
    int64_t games = 0;
    for (int32_t g = 0; g < G; ++g) {
        std::printf("S %d D %d A %d %s: group %d games %lld samples %lld launches %lld\n", S, D, A, aos ? "aos" : "soa", g, (long long)group[g].games,
                    (long long)group[g].samples, (long long)group[g].launches);
        games += group[g].games;
    }
    return games > 0 ? 0 : 1;
}

}  // namespace

int main() {
    int rc = run(257, 3, 27, 1, true, true, 40, 300);
    rc |= run(65, 3, 14, 2, false, true, 40, 100);
    rc |= run(1, 3, 7, 1, false, false, 40, 2);
    return rc;
}
