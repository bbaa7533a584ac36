// ppenv_ppo.hip — the PPO minibatch tail on the device (include/ppenv_ppo.h): the loss gradient, the gradient-norm clip, Adam and the
// dynamic loss scale.
//
// The loss is rl_games' a2c_continuous (restated from its published a2c_continuous.py / common_losses.py; rl_games is absent offline,
// parity unpinned):
//     nlp      = 0.5 sum_j ((a_j - mu_j) / sigma_j)^2 + 0.5 log(2 pi) A + sum_j logstd_j,     sigma = exp(logstd)
//     ratio    = exp(old_nlp - nlp)
//     a_loss   = max(-adv ratio, -adv clamp(ratio, 1 - e, 1 + e))
//     c_loss   = max((v - r)^2, (old_v + clamp(v - old_v, -e, e) - r)^2)     (clip_value; else (v - r)^2)
//     b_loss   = sum_j max(mu_j - 1.1, 0)^2 + min(mu_j + 1.1, 0)^2
//     entropy  = sum_j 0.5 + 0.5 log(2 pi) + logstd_j
//     loss     = mean(a_loss) + 0.5 critic_coef mean(c_loss) - entropy_coef entropy + bounds_loss_coef mean(b_loss)
// Where torch.max meets a tie (ratio inside the clip range; |v - old_v| <= e) both branches carry the same gradient, so the branch
// taken on `>=` is the derivative autograd gives.  The row's log-probability and ratio are formed in fp64, sigma included (nlp is a
// difference of sums of about 30 in fp32 otherwise, of 1e4 and more once mu has run away from the actions); everything written is fp32.
//
// -ffinite-math-only is NOT in this unit's flags (isaacgym_amd/_lib.py): the optimizer's skip depends on seeing an inf / nan norm.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ppenv.h"
#include "../../include/ppenv_ppo.h"
#include "ppenv_reduce_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kLossThreads = 256;                 // 4 waves, one row per lane
constexpr int kOptThreads = 256;
constexpr int PS = PPENV_PPO_PARTIAL_STRIDE;
constexpr double kHalfLog2Pi = 0.91893853320467274178;
constexpr float kMinNormal = 0x1p-126f;           // the smallest scale whose reciprocal is finite whether or not denormals are flushed
constexpr float kMaxFinite = 0x1.fffffep+127f;

// ---- loss gradient: one lane per row, one partial row per workgroup -------------------------------------------------------------
__global__ void __launch_bounds__(kLossThreads) ppo_loss_grad_kernel(ppenv_ppo_loss_args p) {
    __shared__ float wsum[kLossThreads / 64][PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x * kLossThreads + tid;
    const bool valid = row < p.m;
    const int r = valid ? row : 0;                // invalid lanes compute on row 0 and contribute zeros
    const int A = p.a;
    const float scale = *p.scale;
    const float inv_m = 1.0f / (float)p.m;
    const float* mu = p.mu + (size_t)r * p.ld_mu;
    const float* act = p.actions + (size_t)r * p.ld_actions;
    const float* omu = p.old_mu + (size_t)r * p.ld_old_mu;

    double nlp = kHalfLog2Pi * A;
    float kl = 0.0f, bl = 0.0f;
    for (int j = 0; j < A; ++j) {
        const float ls = p.logstd[j], sg = expf(ls), osg = p.old_sigma[j];
        const float m = mu[j];
        // sigma in fp64 as well: with mu far from the actions z^2 reaches 1e4 and more, and the 1e-7 of an fp32 sigma then moves nlp by 1e-2,
        // the ratio with it (tests/test_ppo_runaway_gpu.py)
        const double z = ((double)act[j] - (double)m) / exp((double)ls);
        nlp += 0.5 * z * z + (double)ls;
        const float dm = omu[j] - m;
        kl += logf(osg / sg + 1e-5f) + (sg * sg + dm * dm) / (2.0f * (osg * osg + 1e-5f)) - 0.5f;
        const float hi = fmaxf(m - p.soft_bound, 0.0f), lo = fminf(m + p.soft_bound, 0.0f);
        bl += hi * hi + lo * lo;
    }
    const float adv = p.advantages[r];
    const float ratio = (float)exp((double)p.old_neglogp[r] - nlp);
    const float rc = fminf(fmaxf(ratio, 1.0f - p.e_clip), 1.0f + p.e_clip);
    const float s1 = -adv * ratio, s2 = -adv * rc;
    const float al = fmaxf(s1, s2);
    const float g = (s1 >= s2) ? adv * ratio : 0.0f;             // d a_loss / d nlp
    const float clipped = fabsf(ratio - 1.0f) > p.e_clip ? 1.0f : 0.0f;

    const float v = p.value[(size_t)r * p.ld_value], ov = p.old_values[r], ret = p.returns[r];
    const float cu = (v - ret) * (v - ret);
    float cl = cu, dv = 2.0f * (v - ret);
    if (p.clip_value) {
        const float d = v - ov;
        const float vc = ov + fminf(fmaxf(d, -p.e_clip), p.e_clip);
        const float cc = (vc - ret) * (vc - ret);
        cl = fmaxf(cu, cc);
        if (!(cu >= cc))                                         // the clipped branch: slope 1 inside the clamp's range (where vc is v up to
            dv = (d >= -p.e_clip && d <= p.e_clip) ? 2.0f * (vc - ret) : 0.0f;     // rounding), 0 outside
    }
    const float gs = scale * inv_m;
    if (valid) {
        float* dh = p.d_head + (size_t)row * p.ld_d_head;
        for (int j = 0; j < A; ++j) {
            const float sg = expf(p.logstd[j]), m = mu[j];
            const float zs = (act[j] - m) / (sg * sg);               // -(d nlp / d mu)
            const float db = 2.0f * fmaxf(m - p.soft_bound, 0.0f) + 2.0f * fminf(m + p.soft_bound, 0.0f);
            dh[j] = gs * (-g * zs + p.bounds_loss_coef * db);
        }
        dh[A] = gs * 0.5f * p.critic_coef * dv;
    }
    // d logstd (unscaled, un-averaged): sum over rows of g (1 - z^2)
    for (int j = 0; j < A; ++j) {
        float t = 0.0f;
        if (valid) {
            const float sg = expf(p.logstd[j]);
            const float z = (act[j] - mu[j]) / sg;
            t = g * (1.0f - z * z);
        }
        pp::wave_butterfly(t, pp::add());
        if (lane == 0) wsum[wave][j] = t;
    }
    const float terms[5] = {al, cl, bl, kl, clipped};
    for (int k = 0; k < 5; ++k) {
        float t = valid ? terms[k] : 0.0f;
        pp::wave_butterfly(t, pp::add());
        if (lane == 0) wsum[wave][PPENV_PPO_MAX_ACTIONS + k] = t;
    }
    __syncthreads();
    if (tid < PS) {
        float s = 0.0f;
        const bool used = tid < A || (tid >= PPENV_PPO_MAX_ACTIONS && tid < PPENV_PPO_MAX_ACTIONS + 5);
        if (used)
            for (int w = 0; w < kLossThreads / 64; ++w) s += wsum[w][tid];
        p.partial[(size_t)blockIdx.x * PS + tid] = s;
    }
}

// the partial rows in a fixed order (fp64) -> d logstd, the minibatch means
__global__ void __launch_bounds__(64) ppo_loss_reduce_kernel(ppenv_ppo_loss_args p, int parts) {
    const int tid = threadIdx.x;
    __shared__ double tot[PS];
    if (tid < PS) {
        double s = 0.0;
        for (int b = 0; b < parts; ++b) s += (double)p.partial[(size_t)b * PS + tid];
        tot[tid] = s;
    }
    __syncthreads();
    const double scale = (double)*p.scale, inv_m = 1.0 / (double)p.m;
    if (tid < p.a) p.d_logstd[tid] = (float)(scale * inv_m * tot[tid] - scale * (double)p.entropy_coef);
    if (tid == 0) {
        double ent = 0.0;
        for (int j = 0; j < p.a; ++j) ent += 0.5 + kHalfLog2Pi + (double)p.logstd[j];
        const double al = tot[PPENV_PPO_MAX_ACTIONS] * inv_m, cl = tot[PPENV_PPO_MAX_ACTIONS + 1] * inv_m, bl = tot[PPENV_PPO_MAX_ACTIONS + 2] * inv_m;
        p.stats[PPENV_PPO_LOSS] = (float)(al + 0.5 * p.critic_coef * cl - p.entropy_coef * ent + p.bounds_loss_coef * bl);
        p.stats[PPENV_PPO_A_LOSS] = (float)al;
        p.stats[PPENV_PPO_C_LOSS] = (float)cl;
        p.stats[PPENV_PPO_B_LOSS] = (float)bl;
        p.stats[PPENV_PPO_ENTROPY] = (float)ent;
        p.stats[PPENV_PPO_KL] = (float)(tot[PPENV_PPO_MAX_ACTIONS + 3] * inv_m);
        p.stats[PPENV_PPO_CLIP_FRAC] = (float)(tot[PPENV_PPO_MAX_ACTIONS + 4] * inv_m);
        p.stats[7] = 0.0f;
    }
}

// ---- the multi-tensor passes ---------------------------------------------------------------------------------------------------
// The tensors' items (16-byte vectors of 4 floats where the layout allows, single floats otherwise) form one index space, row-major
// within a tensor; a workgroup-strided loop walks it, so consecutive lanes touch consecutive addresses of one row.
struct Table {
    long long start[PPENV_PPO_MAX_TENSORS + 1];
    int per_row[PPENV_PPO_MAX_TENSORS];
    int vec[PPENV_PPO_MAX_TENSORS];
};

__device__ void load_table(const ppenv_ppo_tensor* t, int count, Table& s) {
    if (threadIdx.x == 0) {
        long long at = 0;
        for (int i = 0; i < count; ++i) {
            const ppenv_ppo_tensor d = t[i];
            const uintptr_t bits = reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.g) | reinterpret_cast<uintptr_t>(d.m) |
                                   reinterpret_cast<uintptr_t>(d.v);
            const int vec = (d.cols % 4 == 0 && d.ld_p % 4 == 0 && d.ld_g % 4 == 0 && (bits & 15) == 0) ? 1 : 0;
            s.vec[i] = vec;
            s.per_row[i] = vec ? d.cols / 4 : d.cols;
            s.start[i] = at;
            at += (long long)d.rows * s.per_row[i];
        }
        s.start[count] = at;
    }
    __syncthreads();
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    pp::wave_butterfly(v, pp::add());
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kOptThreads / 64; ++w) s += red[w];
    __syncthreads();
    return s;                                     // every thread: the same value, summed in the same order
}

__global__ void __launch_bounds__(kOptThreads) ppo_grad_sumsq_kernel(const ppenv_ppo_tensor* table, int count, double* slab) {
    __shared__ Table s;
    __shared__ double red[kOptThreads / 64];
    load_table(table, count, s);
    const long long total = s.start[count], stride = (long long)gridDim.x * kOptThreads;
    double acc = 0.0;
    int t = 0;
    for (long long it = (long long)blockIdx.x * kOptThreads + threadIdx.x; it < total; it += stride) {
        while (it >= s.start[t + 1]) ++t;
        const ppenv_ppo_tensor d = table[t];
        const long long i = it - s.start[t];
        const int r = (int)(i / s.per_row[t]), c = (int)(i % s.per_row[t]);
        if (s.vec[t]) {
            const float4 g = *reinterpret_cast<const float4*>(d.g + (size_t)r * d.ld_g + 4 * c);
            acc += (double)g.x * g.x + (double)g.y * g.y + (double)g.z * g.z + (double)g.w * g.w;
        } else {
            const double g = d.g[(size_t)r * d.ld_g + c];
            acc += g * g;
        }
    }
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) slab[blockIdx.x] = sum;
}

__device__ __forceinline__ bool finite64(double x) {
    return (__double_as_longlong(x) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

struct AdamCoef { float gmul, b1, b2, one_m_b1, one_m_b2, step_size, bc2_sqrt, eps, world; bool mean; };

// Every rounding is spelled out (contraction off, the fused steps written as fma): left to the compiler, the two products of the second
// moment were fused differently in the 16-byte loop and in the element loop, and a tensor's bits depended on its alignment and strides
// (tests/test_ppo_edges_gpu.py::test_adam_layouts_agree_bitwise_and_match_torch).
__device__ __forceinline__ void adam1(float& p, float& m, float& v, float g, const AdamCoef& k) {
    #pragma clang fp contract(off)
    if (k.mean) g = g / k.world;                                  // the rank mean of an all-reduced sum: all_grads / world_size (IEEE division)
    g *= k.gmul;                                                  // unscale and clip: rounded, as torch's in-place unscale leaves the gradient
    m = __builtin_fmaf(k.one_m_b1, g - m, m);                     // exp_avg.lerp_(grad, 1 - beta1)
    v = __builtin_fmaf(k.one_m_b2 * g, g, v * k.b2);              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = __builtin_fmaf(-k.step_size, m / denom, p);               // param.addcdiv_(exp_avg, denom, -step_size)
}

__global__ void __launch_bounds__(kOptThreads) ppo_adam_kernel(const ppenv_ppo_tensor* table, int count, const double* slab, int parts,
                                                               ppenv_ppo_adam hp, const float* lr, const ppenv_ppo_scaler* state_in,
                                                               ppenv_ppo_scaler* state_out) {
    __shared__ Table s;
    __shared__ double red[kOptThreads / 64];
    double part = 0.0;
    for (int b = threadIdx.x; b < parts; b += kOptThreads) part += slab[b];
    const bool mean = hp.world > 1;
    // the rank means' square sum: the sums' over world^2, in fp64 (exact for a power-of-two world: identical shards then reproduce one rank)
    const double raw = block_sum(part, red);
    const double sumsq = mean ? raw / ((double)hp.world * (double)hp.world) : raw;
    const ppenv_ppo_scaler st = *state_in;
    // The step is taken on a finite square sum AND a scale that can be divided out: a normal positive number (`>=` is false for a NaN).  At 0
    // or a denormal — a state loaded from a run whose scale had no floor — the scaled gradients are all 0 or denormal, 1 / scale is inf
    // (or the gradients are flushed), and g x gmul = 0 x inf would put a NaN into every parameter: skipped instead, and the scale lifted below.
    const bool finite = finite64(sumsq) && st.scale >= kMinNormal;
    const double norm = sqrt(sumsq) / (double)st.scale;            // of the unscaled gradients
    if (blockIdx.x == 0 && threadIdx.x == 0) {                   // GradScaler.update with the two bounds of include/ppenv_ppo.h, into the OTHER buffer
        ppenv_ppo_scaler nx = st;
        nx.grad_norm = (float)norm;
        if (!finite) {
            nx.scale = st.scale * hp.backoff_factor;
            nx.growth_tracker = 0;
            nx.skipped = st.skipped + 1;
        } else {
            nx.step = st.step + 1;
            nx.growth_tracker = st.growth_tracker + 1;
            if (nx.growth_tracker >= hp.growth_interval) {
                const float grown = st.scale * hp.growth_factor;
                if (fabsf(grown) <= kMaxFinite) nx.scale = grown;    // withheld where the product is inf: at inf every later step would be skipped
                nx.growth_tracker = 0;
            }
        }
        if (hp.backoff_factor < 1.0f && !(nx.scale >= PPENV_PPO_SCALE_FLOOR)) {     // a dynamic scale: never below the floor (a NaN is lifted too)
            nx.scale = PPENV_PPO_SCALE_FLOOR;
            nx.reserved[0] = st.reserved[0] + 1;
        }
        *state_out = nx;
    }
    if (!finite) return;                                          // GradScaler.step: parameters and moments untouched
    load_table(table, count, s);
    const float coef = hp.truncate ? fminf(1.0f, hp.max_norm / ((float)norm + 1e-6f)) : 1.0f;     // clip_grad_norm_
    const int step = st.step + 1;
    const double bc1 = 1.0 - pow(hp.beta1, step), bc2 = 1.0 - pow(hp.beta2, step);
    AdamCoef k;
    k.gmul = (1.0f / st.scale) * coef;
    k.b1 = (float)hp.beta1; k.b2 = (float)hp.beta2; k.one_m_b1 = (float)(1.0 - hp.beta1); k.one_m_b2 = (float)(1.0 - hp.beta2);
    k.step_size = (float)((double)*lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.eps = hp.eps;
    k.world = (float)hp.world;
    k.mean = mean;
    const long long total = s.start[count], stride = (long long)gridDim.x * kOptThreads;
    int t = 0;
    for (long long it = (long long)blockIdx.x * kOptThreads + threadIdx.x; it < total; it += stride) {
        while (it >= s.start[t + 1]) ++t;
        const ppenv_ppo_tensor d = table[t];
        const long long i = it - s.start[t];
        const int r = (int)(i / s.per_row[t]), c = (int)(i % s.per_row[t]);
        if (s.vec[t]) {
            float4* pp = reinterpret_cast<float4*>(d.p + (size_t)r * d.ld_p + 4 * c);
            float4* mp = reinterpret_cast<float4*>(d.m + (size_t)r * d.cols + 4 * c);
            float4* vp = reinterpret_cast<float4*>(d.v + (size_t)r * d.cols + 4 * c);
            const float4 g = *reinterpret_cast<const float4*>(d.g + (size_t)r * d.ld_g + 4 * c);
            float4 P = *pp, M = *mp, V = *vp;
            adam1(P.x, M.x, V.x, g.x, k); adam1(P.y, M.y, V.y, g.y, k); adam1(P.z, M.z, V.z, g.z, k); adam1(P.w, M.w, V.w, g.w, k);
            *pp = P; *mp = M; *vp = V;
        } else {
            float& P = d.p[(size_t)r * d.ld_p + c];
            float& M = d.m[(size_t)r * d.cols + c];
            float& V = d.v[(size_t)r * d.cols + c];
            float pv = P, mv = M, vv = V;
            adam1(pv, mv, vv, d.g[(size_t)r * d.ld_g + c], k);
            P = pv; M = mv; V = vv;
        }
    }
}

}  // namespace

extern "C" size_t ppenv_ppo_loss_partial_floats(int32_t m) {
    return m > 0 ? (size_t)((m + kLossThreads - 1) / kLossThreads) * PS : 0;
}

extern "C" int ppenv_ppo_loss_grad(const ppenv_ppo_loss_args* a, void* stream) {
    const bool ok = a && a->m > 0 && a->a > 0 && a->a <= PPENV_PPO_MAX_ACTIONS && a->mu && a->value && a->actions && a->old_mu && a->old_sigma &&
                    a->old_neglogp && a->advantages && a->old_values && a->returns && a->logstd && a->scale && a->d_head && a->d_logstd && a->stats &&
                    a->partial && a->ld_mu >= a->a && a->ld_value >= 1 && a->ld_actions >= a->a && a->ld_old_mu >= a->a && a->ld_d_head >= a->a + 1;
    if (!ok) {
        ppenv_set_error("ppenv_ppo_loss_grad: NULL pointer or inconsistent sizes (need 0 < a <= 32, row strides >= a, ld_d_head >= a + 1)");
        return PPENV_EINVAL;
    }
    const int parts = (a->m + kLossThreads - 1) / kLossThreads;
    hipLaunchKernelGGL(ppo_loss_grad_kernel, dim3(parts), dim3(kLossThreads), 0, (hipStream_t)stream, *a);
    if (int rc = pp_launched("launching ppo_loss_grad_kernel failed")) return rc;
    hipLaunchKernelGGL(ppo_loss_reduce_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a, parts);
    return pp_launched("launching ppo_loss_reduce_kernel failed");
}

extern "C" int ppenv_ppo_grad_sumsq(const ppenv_ppo_tensor* table, int32_t count, double* slab, int32_t parts, void* stream) {
    if (!table || !slab || count <= 0 || count > PPENV_PPO_MAX_TENSORS || parts <= 0 || parts > 65535) {
        ppenv_set_error("ppenv_ppo_grad_sumsq: NULL pointer, 0 < count <= 64 tensors, 0 < parts <= 65535");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(ppo_grad_sumsq_kernel, dim3(parts), dim3(kOptThreads), 0, (hipStream_t)stream, table, count, slab);
    return pp_launched("launching ppo_grad_sumsq_kernel failed");
}

extern "C" int ppenv_ppo_adam_step(const ppenv_ppo_tensor* table, int32_t count, const double* slab, int32_t parts, ppenv_ppo_adam hp, const float* lr,
                                   const ppenv_ppo_scaler* state_in, ppenv_ppo_scaler* state_out, void* stream) {
    if (!table || !slab || !lr || !state_in || !state_out || state_in == state_out || count <= 0 || count > PPENV_PPO_MAX_TENSORS || parts <= 0 ||
        parts > 65535 || hp.growth_interval <= 0 || hp.world < 0) {
        ppenv_set_error("ppenv_ppo_adam_step: NULL pointer, state_in == state_out (the state is double-buffered), bad sizes or world < 0");
        return PPENV_EINVAL;
    }
    hipLaunchKernelGGL(ppo_adam_kernel, dim3(parts), dim3(kOptThreads), 0, (hipStream_t)stream, table, count, slab, parts, hp, lr, state_in, state_out);
    return pp_launched("launching ppo_adam_kernel failed");
}
