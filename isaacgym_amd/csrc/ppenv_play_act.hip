// ppenv_play_act.hip — actuator usage accounting of a played checkpoint, on the device (include/ppenv_play_act.h): per env a running
// episode of per-joint torque / speed / position / power / action figures, folded into per-group, per-joint totals when the env finishes a
// game, under ppenv_play.hip's freeze and in its launch shape.
//
//   play_act_rows_kernel     workgroup (x, y) is chunk x of group y (chunks of 256 envs counted from the group's first env, the ragged
//                            last one guarded); a lane owns one env: a sample (the dof loop of ppenv_play_act_device.h) or a fold.  The
//                            folds of the workgroup are summed in a fixed order — xor butterfly within a wave (strides 1 up to 32, four of
//                            the six stages as DPP row operations: wave_merge), the four waves in order through LDS — into ONE partial: a
//                            pp_play_act_group and D pp_play_act_joint.  (The other accounting kernels share ppenv_reduce_device.h, whose
//                            butterfly runs 32 down to 1 through permutes; this unit keeps its own exchange for the DPP stages.)  A workgroup in which no env
//                            finished skips all of that and writes the empty partial (a uniform branch: __syncthreads_or).
//   play_act_totals_kernel   one workgroup per group, one wave per three dofs: lane l sums the group's partials l, l + 64, ... of the wave's
//                            dofs in order, a butterfly, a lane adds the result to joint[g * D + d]; wave 0 does the same for group[g]
//                            after a barrier (every wave tests its games first); a launch without a finished game only counts itself.
// Reads group[g].games for the freeze in both; only the second writes the totals, and workgroup g of it touches group g's alone.  No atomics.
//
// Memory.  The running state is plane-major ([1 + 10 D][N] words): lane = env, so every state access is a coalesced 256-byte row per
// wave, and that is 20 of the ~24 words a dof costs.  The inputs are read where the env keeps them: the 7-dof SoA [D][N] is coalesced
// too; the 27-dof AoS (dof_states [N, 27, 2], dof_force [N, 27], actions [N, 27]) is read with a per-lane stride of 216 / 108 bytes —
// a wave's load touches 64 rows, but the dof loop walks each row's lines front to back, so every fetched line is used whole from L1 / L2
// within the same loop and HBM traffic stays the tensors' size (~1.8 MB at 4096 envs).  Staging the rows through LDS would buy
// coalescing for a kernel that is bound by its two launches, not by these bytes (DESIGN §5e has the timings).
//
// This unit's flags (isaacgym_amd/_lib.py): -ffp-contract=off, signed zeros kept, no -ffinite-math-only (max_exc starts at -inf).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_play_act_device.h"

#include "ppenv_play_host.h"

namespace {

constexpr int kBlock = PPENV_PLAY_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kFold = 3;                                         // dofs whose folds run side by side in play_act_rows_kernel
constexpr int kTotalsBlock = 64 * ((PP_PLAY_ACT_MAX_DOF + kFold - 1) / kFold);      // play_act_totals_kernel: at most one wave per kFold dofs
constexpr int kResetBlocks = 4096;                              // the reset's grid-stride cap

// The xor butterfly runs from stride 1 up to 32.  Every lane ends with the same sums: at each stage both partners form a + b and b + a,
// which are the same bits — so after the strides below `off` all lanes of an aligned group of `off` lanes hold the same bits, and the
// partner l ^ off may be replaced by ANY lane of the partner's group.  That is what lets four of the six stages be DPP row operations
// (full-rate vector moves) instead of LDS-crossbar permutes: strides 1 and 2 are quad permutes (exactly l ^ off); stride 4 is the
// mirror of a half row (l -> 7 - l) and stride 8 the mirror of a row (l -> 15 - l), both lanes of the partner's group.
template <int kOff>
__device__ __forceinline__ int partner_word(int v) {
    if constexpr (kOff == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);          // quad_perm [1, 0, 3, 2]
    else if constexpr (kOff == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);     // quad_perm [2, 3, 0, 1]
    else if constexpr (kOff == 4) return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);    // row_half_mirror
    else if constexpr (kOff == 8) return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);    // row_mirror
    else return __shfl_xor(v, kOff, 64);
}

template <int kOff, class T>
__device__ __forceinline__ T partner(T v) {
    static_assert(sizeof(T) % sizeof(int) == 0, "whole words");
    int w[sizeof(T) / sizeof(int)];
    __builtin_memcpy(w, &v, sizeof(T));
    #pragma unroll
    for (unsigned i = 0; i < sizeof(T) / sizeof(int); ++i) w[i] = partner_word<kOff>(w[i]);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

template <int kOff>
__device__ __forceinline__ void merge_stage(pp_play_act_group& p) {
    pp_play_act_group o;
    o.games = partner<kOff>(p.games);
    o.samples = partner<kOff>(p.samples);
    o.energy = partner<kOff>(p.energy);
    o.energy_sq = partner<kOff>(p.energy_sq);
    pp::act_group_merge(p, o);
}

__device__ __forceinline__ void wave_merge(pp_play_act_group& p) {
    merge_stage<1>(p);
    merge_stage<2>(p);
    merge_stage<4>(p);
    merge_stage<8>(p);
    merge_stage<16>(p);
    merge_stage<32>(p);
}

// ... of K joints at once: a stage's moves are all issued before the first sum needs one.
template <int kOff, int K>
__device__ __forceinline__ void merge_stage(pp_play_act_joint (&p)[K]) {
    pp_play_act_joint o[K];
    #pragma unroll
    for (int k = 0; k < K; ++k) {
        o[k].c_effort = partner<kOff>(p[k].c_effort);
        o[k].c_vel = partner<kOff>(p[k].c_vel);
        o[k].c_limit = partner<kOff>(p[k].c_limit);
        o[k].c_clip = partner<kOff>(p[k].c_clip);
        o[k].abs_tau = partner<kOff>(p[k].abs_tau);
        o[k].tau_sq = partner<kOff>(p[k].tau_sq);
        o[k].power = partner<kOff>(p[k].power);
        o[k].max_abs_tau = partner<kOff>(p[k].max_abs_tau);
        o[k].max_abs_vel = partner<kOff>(p[k].max_abs_vel);
        o[k].max_exc = partner<kOff>(p[k].max_exc);
    }
    #pragma unroll
    for (int k = 0; k < K; ++k) pp::act_joint_merge(p[k], o[k]);
}

template <int K>
__device__ __forceinline__ void wave_merge(pp_play_act_joint (&p)[K]) {
    merge_stage<1>(p);
    merge_stage<2>(p);
    merge_stage<4>(p);
    merge_stage<8>(p);
    merge_stage<16>(p);
    merge_stage<32>(p);
}

// Workgroup (x, y) is chunk x of group y: a workgroup belongs to one group, so the freeze test is uniform in it.
__global__ __launch_bounds__(kBlock) void play_act_rows_kernel(pp_play_act_inputs in, const int64_t* __restrict__ done, int32_t envs_per_group, int32_t parts,
                                                               int32_t num_agents, int32_t num_dofs, int64_t num_envs, int64_t games_num,
                                                               const pp_play_act_limit* __restrict__ limits, pp_play_act_thresholds thr, void* state,
                                                               const pp_play_act_group* __restrict__ group, pp_play_act_group* __restrict__ gpart,
                                                               pp_play_act_joint* __restrict__ jpart) {
    __shared__ pp_play_act_group wave_group[kWaves];
    __shared__ pp_play_act_joint wave_joint[PP_PLAY_ACT_MAX_DOF][kWaves];
    const int32_t g = (int32_t)blockIdx.y, chunk = (int32_t)blockIdx.x;
    if (pp::act_frozen(group[g].games, games_num)) return;       // uniform: the whole workgroup leaves (its partial is not read either)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t local = chunk * kBlock + tid;                  // the env's index within its group
    const bool live = local < envs_per_group;
    const int64_t e = (int64_t)g * envs_per_group + local;
    const bool fin = live && done[(size_t)num_agents * (size_t)e] != 0;      // all 64 bits
    if (live && !fin) pp::act_sample(e, num_envs, num_dofs, in, limits, thr, state);
    const size_t slot = (size_t)g * parts + chunk;
    if (!__syncthreads_or(fin ? 1 : 0)) {                        // uniform: nobody finished, the partial is the empty one
        if (tid == 0) {
            pp_play_act_group s;
            pp::act_group_clear(s);
            gpart[slot] = s;
        }
        if (tid < num_dofs) {
            pp_play_act_joint s;
            pp::act_joint_clear(s);
            jpart[slot * num_dofs + tid] = s;
        }
        return;
    }
    pp_play_act_group ga;
    pp::act_group_clear(ga);
    int32_t n = 0;
    if (fin) n = pp::act_fold_env(e, num_envs, num_dofs, state, ga);
    wave_merge(ga);
    if (lane == 0) wave_group[wave] = ga;
    // kFold dofs at a time: their butterflies are independent and interleave, and the next kFold dofs' words are loaded before these are
    // summed — otherwise every dof pays a memory round trip and six dependent shuffle stages of its own
    pp::act_joint_words cur[kFold], next[kFold];
    #pragma unroll
    for (int k = 0; k < kFold; ++k)
        if (fin && k < num_dofs) pp::act_fold_load(e, num_envs, num_dofs, k, state, cur[k]);
    for (int32_t d0 = 0; d0 < num_dofs; d0 += kFold) {
        #pragma unroll
        for (int k = 0; k < kFold; ++k)
            if (fin && d0 + kFold + k < num_dofs) pp::act_fold_load(e, num_envs, num_dofs, d0 + kFold + k, state, next[k]);
        pp_play_act_joint ja[kFold];
        #pragma unroll
        for (int k = 0; k < kFold; ++k) {
            pp::act_joint_clear(ja[k]);
            if (fin && d0 + k < num_dofs) {
                pp::act_fold_joint(cur[k], n, ja[k]);
                pp::act_fold_zero(e, num_envs, num_dofs, d0 + k, state);
            }
        }
        wave_merge(ja);
        #pragma unroll
        for (int k = 0; k < kFold; ++k) {
            if (lane == 0 && d0 + k < num_dofs) wave_joint[d0 + k][wave] = ja[k];
            cur[k] = next[k];
        }
    }
    __syncthreads();
    if (tid == 0) {
        pp_play_act_group s = wave_group[0];
        for (int w = 1; w < kWaves; ++w) pp::act_group_merge(s, wave_group[w]);
        gpart[slot] = s;
    }
    if (tid < num_dofs) {
        pp_play_act_joint s = wave_joint[tid][0];
        for (int w = 1; w < kWaves; ++w) pp::act_joint_merge(s, wave_joint[tid][w]);
        jpart[slot * num_dofs + tid] = s;
    }
}

// Workgroup g is group g; wave w of it owns the dofs kFold * w .. kFold * w + kFold - 1 (the launch has one wave per kFold dofs).
__global__ __launch_bounds__(kTotalsBlock) void play_act_totals_kernel(const pp_play_act_group* __restrict__ gpart, const pp_play_act_joint* __restrict__ jpart,
                                                                       int32_t parts, int32_t num_dofs, int64_t games_num,
                                                                       pp_play_act_group* __restrict__ group, pp_play_act_joint* __restrict__ joint) {
    const int32_t g = (int32_t)blockIdx.x;
    if (pp::act_frozen(group[g].games, games_num)) return;       // the word the group's chunks tested: nothing wrote it in between
    const size_t first = (size_t)g * parts;
    pp_play_act_group ga;
    pp::act_group_clear(ga);
    const int lane = (int)(threadIdx.x & 63);
    for (int32_t b = lane; b < parts; b += 64) pp::act_group_merge(ga, gpart[first + b]);     // every wave sums the group's own partials: the same bits
    wave_merge(ga);
    __syncthreads();                                             // every wave has tested group[g].games: wave 0 may now write it
    if (threadIdx.x == 0) {
        pp_play_act_group t = group[g];
        pp::act_group_add(t, ga);
        group[g] = t;
    }
    if (ga.games == 0) return;                                   // uniform (every lane holds the same sums): the joints' partials are all empty
    // wave w owns the dofs kFold * w ..: their partials gathered, their totals on the way during the butterflies; lane k adds dof d0 + k
    // (every lane holds the same sums)
    const int32_t d0 = kFold * (int32_t)(threadIdx.x >> 6);
    pp_play_act_joint sum[kFold];
    #pragma unroll
    for (int k = 0; k < kFold; ++k) {
        pp::act_joint_clear(sum[k]);
        if (d0 + k < num_dofs)
            for (int32_t b = lane; b < parts; b += 64) pp::act_joint_merge(sum[k], jpart[(first + b) * num_dofs + d0 + k]);
    }
    const bool own = lane < kFold && d0 + lane < num_dofs;
    pp_play_act_joint t;
    pp::act_joint_clear(t);
    if (own) t = joint[(size_t)g * num_dofs + d0 + lane];
    wave_merge(sum);
    #pragma unroll
    for (int k = 0; k < kFold; ++k) {
        if (own && lane == k) {
            pp::act_joint_merge(t, sum[k]);
            joint[(size_t)g * num_dofs + d0 + k] = t;
        }
    }
}

__global__ __launch_bounds__(kBlock) void play_act_reset_kernel(int64_t words, int32_t groups, int32_t joints, uint32_t* __restrict__ state,
                                                                pp_play_act_group* __restrict__ group, pp_play_act_joint* __restrict__ joint) {
    const int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = i0; i < words; i += stride) state[i] = 0u;
    for (int64_t i = i0; i < joints; i += stride) {
        pp_play_act_joint t;
        pp::act_joint_clear(t);
        joint[i] = t;
    }
    for (int64_t i = i0; i < groups; i += stride) {
        pp_play_act_group t;
        pp::act_group_clear(t);
        group[i] = t;
    }
}

bool sizes_ok(int32_t envs_per_group, int32_t groups, int32_t num_agents, int32_t num_dofs) {
    return pp_play_sizes_ok(envs_per_group, groups, num_agents) && num_dofs >= 1 && num_dofs <= PP_PLAY_ACT_MAX_DOF && num_dofs % num_agents == 0;
}

const char kSizes[] = "num_dofs outside 1..32 or no multiple of num_agents, groups outside 1..1024, envs_per_group <= 0, num_agents not 1 or 2, or more than "
                      "2^31 - 1 rows";

}  // namespace

extern "C" size_t pp_play_act_state_bytes(int32_t envs_per_group, int32_t groups, int32_t num_dofs) {
    return sizes_ok(envs_per_group, groups, 1, num_dofs) ? sizeof(uint32_t) * (size_t)(1 + PP_PLAY_ACT_FIELDS * num_dofs) * (size_t)envs_per_group * groups : 0;
}

extern "C" size_t pp_play_act_partial_bytes(int32_t envs_per_group, int32_t groups, int32_t num_dofs) {
    return sizes_ok(envs_per_group, groups, 1, num_dofs)
               ? (size_t)groups * (size_t)pp_blocks_of(envs_per_group, kBlock) * (sizeof(pp_play_act_group) + (size_t)num_dofs * sizeof(pp_play_act_joint))
               : 0;
}

extern "C" int pp_play_act_reset(int32_t envs_per_group, int32_t groups, int32_t num_dofs, void* state, pp_play_act_group* group, pp_play_act_joint* joint,
                                 void* stream) {
    if (!sizes_ok(envs_per_group, groups, 1, num_dofs) || !state || !group || !joint) {
        pp_set_errorf("pp_play_act_reset: NULL pointer, %s", kSizes);
        return PPENV_EINVAL;
    }
    const int64_t words = (int64_t)(1 + PP_PLAY_ACT_FIELDS * num_dofs) * envs_per_group * groups;
    const int64_t blocks = (words + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(play_act_reset_kernel, dim3((uint32_t)(blocks < kResetBlocks ? blocks : kResetBlocks)), dim3(kBlock), 0, (hipStream_t)stream, words,
                       groups, groups * num_dofs, (uint32_t*)state, group, joint);
    return pp_launched("launching play_act_reset_kernel failed");
}

extern "C" int pp_play_act_accumulate(const pp_play_act_inputs* in, const int64_t* done, int32_t envs_per_group, int32_t groups, int32_t num_agents,
                                      int32_t num_dofs, int64_t games_num, const pp_play_act_limit* limits, const pp_play_act_thresholds* thresholds,
                                      void* state, pp_play_act_group* group, pp_play_act_joint* joint, void* partial, void* stream) {
    if (!sizes_ok(envs_per_group, groups, num_agents, num_dofs) || !in || !in->q.p || !in->qd.p || !in->tau.p || !done || !limits || !thresholds || !state ||
        !group || !joint || !partial || games_num < 1) {
        pp_set_errorf("pp_play_act_accumulate: NULL pointer, %s, or games_num < 1", kSizes);
        return PPENV_EINVAL;
    }
    const int32_t parts = pp_blocks_of(envs_per_group, kBlock);  // per group
    pp_play_act_group* gpart = (pp_play_act_group*)partial;      // [G * parts], then the joints' [G * parts * D]: both 8-byte aligned
    pp_play_act_joint* jpart = (pp_play_act_joint*)(gpart + (size_t)groups * parts);
    hipLaunchKernelGGL(play_act_rows_kernel, dim3((uint32_t)parts, (uint32_t)groups), dim3(kBlock), 0, (hipStream_t)stream, *in, done, envs_per_group, parts,
                       num_agents, num_dofs, (int64_t)envs_per_group * groups, games_num, limits, *thresholds, state, group, gpart, jpart);
    if (int rc = pp_launched("launching play_act_rows_kernel failed")) return rc;
    hipLaunchKernelGGL(play_act_totals_kernel, dim3(groups), dim3(64 * ((num_dofs + kFold - 1) / kFold)), 0, (hipStream_t)stream, gpart, jpart, parts, num_dofs, games_num, group, joint);
    return pp_launched("launching play_act_totals_kernel failed");
}
