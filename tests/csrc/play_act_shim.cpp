// play_act_shim.cpp — the actuator-accounting arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_play_act_device.h) compiled for the
// host and summed in the kernels' order, as play_pair_shim.cpp does for the paired statistics.  TEST INFRASTRUCTURE ONLY.  Built by
// tests/play_act_shim_binding.py with -ffp-contract=off and WITHOUT -ffinite-math-only (max_exc starts at -inf).
#include "../../isaacgym_amd/csrc/ppenv_play_act_device.h"
#include "butterfly_host.h"

namespace {

// the per-element functions as callables (PP_HD functions are always inlined: their address cannot be passed)
struct GroupOps {
    void operator()(pp_play_act_group& p) const { pp::act_group_clear(p); }
    void operator()(pp_play_act_group& into, const pp_play_act_group& from) const { pp::act_group_merge(into, from); }
};
struct JointOps {
    void operator()(pp_play_act_joint& p) const { pp::act_joint_clear(p); }
    void operator()(pp_play_act_joint& into, const pp_play_act_joint& from) const { pp::act_joint_merge(into, from); }
};

// play_act_totals_kernel's sum of a group's partials (stride `step` apart): lane l takes l, l + 64, ... in order, then the butterfly.
template <class T, class Ops>
T wave_sum(const T* part, int32_t parts, size_t step, Ops merge) {
    T lane[64];
    for (int l = 0; l < 64; ++l) {
        merge(lane[l]);                                          // with one argument: Ops' clear
        for (int32_t b = l; b < parts; b += 64) merge(lane[l], part[(size_t)b * step]);
    }
    return butterfly::block_sum(lane, 64, butterfly::ascending, merge);
}

}  // namespace

extern "C" {

size_t play_act_shim_sizeof_group() { return sizeof(pp_play_act_group); }
size_t play_act_shim_sizeof_joint() { return sizeof(pp_play_act_joint); }
size_t play_act_shim_sizeof_inputs() { return sizeof(pp_play_act_inputs); }

// pp_play_act_reset on host memory
void play_act_shim_reset(int32_t envs_per_group, int32_t groups, int32_t num_dofs, uint32_t* state, pp_play_act_group* group, pp_play_act_joint* joint) {
    const int64_t words = (int64_t)(1 + PP_PLAY_ACT_FIELDS * num_dofs) * envs_per_group * groups;
    for (int64_t i = 0; i < words; ++i) state[i] = 0u;
    for (int32_t g = 0; g < groups; ++g) pp::act_group_clear(group[g]);
    for (int32_t i = 0; i < groups * num_dofs; ++i) pp::act_joint_clear(joint[i]);
}

// pp_play_act_accumulate on host memory: both kernels, workgroup by workgroup and lane by lane, `partial` laid out as the entry lays it out.
void play_act_shim_accumulate(const pp_play_act_inputs* in, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents,
                              int32_t num_dofs, int64_t games_num, const pp_play_act_limit* limits, const pp_play_act_thresholds* thr, void* state,
                              pp_play_act_group* group, pp_play_act_joint* joint, void* partial) {
    const int32_t parts = (envs_per_group + PPENV_PLAY_BLOCK - 1) / PPENV_PLAY_BLOCK;
    const int64_t num_envs = (int64_t)envs_per_group * groups;
    pp_play_act_group* gpart = (pp_play_act_group*)partial;
    pp_play_act_joint* jpart = (pp_play_act_joint*)(gpart + (size_t)groups * parts);
    for (int32_t g = 0; g < groups; ++g) {                       // play_act_rows_kernel
        if (pp::act_frozen(group[g].games, games_num)) continue;
        for (int32_t chunk = 0; chunk < parts; ++chunk) {
            const size_t slot = (size_t)g * parts + chunk;
            bool fin[PPENV_PLAY_BLOCK], any = false;
            int64_t env[PPENV_PLAY_BLOCK];
            for (int l = 0; l < PPENV_PLAY_BLOCK; ++l) {
                const int32_t local = chunk * PPENV_PLAY_BLOCK + l;
                const bool live = local < envs_per_group;
                env[l] = (int64_t)g * envs_per_group + local;
                fin[l] = live && done[(size_t)num_agents * (size_t)env[l]] != 0;
                if (live && !fin[l]) pp::act_sample(env[l], num_envs, num_dofs, *in, limits, *thr, state);
                any = any || fin[l];
            }
            if (!any) {
                pp::act_group_clear(gpart[slot]);
                for (int32_t d = 0; d < num_dofs; ++d) pp::act_joint_clear(jpart[slot * num_dofs + d]);
                continue;
            }
            pp_play_act_group ga[PPENV_PLAY_BLOCK];
            int32_t n[PPENV_PLAY_BLOCK];
            for (int l = 0; l < PPENV_PLAY_BLOCK; ++l) {
                pp::act_group_clear(ga[l]);
                n[l] = fin[l] ? pp::act_fold_env(env[l], num_envs, num_dofs, state, ga[l]) : 0;
            }
            gpart[slot] = butterfly::block_sum(ga, PPENV_PLAY_BLOCK, butterfly::ascending, GroupOps());     // the waves by the butterfly, strides 1 up to 32, then in order
            for (int32_t d = 0; d < num_dofs; ++d) {
                pp_play_act_joint ja[PPENV_PLAY_BLOCK];
                for (int l = 0; l < PPENV_PLAY_BLOCK; ++l) {
                    pp::act_joint_clear(ja[l]);
                    if (fin[l]) {
                        pp::act_joint_words w;
                        pp::act_fold_load(env[l], num_envs, num_dofs, d, state, w);
                        pp::act_fold_joint(w, n[l], ja[l]);
                        pp::act_fold_zero(env[l], num_envs, num_dofs, d, state);
                    }
                }
                jpart[slot * num_dofs + d] = butterfly::block_sum(ja, PPENV_PLAY_BLOCK, butterfly::ascending, JointOps());
            }
        }
    }
    for (int32_t g = 0; g < groups; ++g) {                       // play_act_totals_kernel
        if (pp::act_frozen(group[g].games, games_num)) continue;
        const size_t first = (size_t)g * parts;
        const pp_play_act_group ga = wave_sum(gpart + first, parts, 1, GroupOps());
        pp::act_group_add(group[g], ga);
        if (ga.games == 0) continue;
        for (int32_t d = 0; d < num_dofs; ++d)
            pp::act_joint_merge(joint[(size_t)g * num_dofs + d],
                                wave_sum(jpart + first * num_dofs + d, parts, (size_t)num_dofs, JointOps()));
    }
}

}
