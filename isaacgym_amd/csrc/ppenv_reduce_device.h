// ppenv_reduce_device.h — the fixed summation order of the play, paired-difference, score-meter and PPO-tail kernels, once: an xor
// butterfly within a wave, strides 32 down to 1, then the waves of a workgroup in order through LDS.  Internal and device-only: no part
// of the ABI (include/*.h state the order in words; tests/csrc/butterfly_host.h walks it on plain arrays for the host builds).  Templates
// only: every unit compiles it under its own contraction and finite-math flags.
//
// Every lane ends with the same sums: at each stage both partners form a + b and b + a, which are the same bits.  Which bits depends on
// the order of the stages, so the order is part of a kernel's contract.  In this order every stage must be a true l ^ off permute.
// (ppenv_play_act.hip runs its butterfly from stride 1 up, where four stages may be DPP row operations, and keeps its own exchange: moved
// here as whole structs, play_act_rows_kernel measured 1 % slower than with its fields listed.)
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace pp {

// The value of lane l ^ off, unit by unit and with no field named, so a field added to T travels along (padding and reserved words
// too: the ones a merge never reads are dead moves, which the compiler drops).  The units are 8 bytes where T is 8-byte aligned: moved as
// single words, an int64 field comes back as lo | hi << 32, and the merge's 64-bit add is re-associated into two.
template <class T>
__device__ __forceinline__ T partner(T v, int off) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % sizeof(int) == 0, "moved as whole words");
    using unit = std::conditional_t<sizeof(T) % 8 == 0 && alignof(T) % 8 == 0, long long, int>;
    unit u[sizeof(T) / sizeof(unit)];
    __builtin_memcpy(u, &v, sizeof(T));
    #pragma unroll
    for (unsigned i = 0; i < sizeof(T) / sizeof(unit); ++i) u[i] = __shfl_xor(u[i], off, 64);
    __builtin_memcpy(&v, u, sizeof(T));
    return v;
}

// The butterfly of a wave, merge(into, from) per stage; every lane ends with the wave's sum.
template <class T, class Merge>
__device__ __forceinline__ void wave_butterfly(T& p, Merge merge) {
    #pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = partner(p, off);
        merge(p, o);
    }
}

// The scalars' merge.
struct add { template <class T> __device__ __forceinline__ void operator()(T& into, const T& from) const { into += from; } };

// The workgroup tail in its pieces: lane 0 of each wave leaves the wave's sum in the caller's __shared__ part[kWaves]; after a barrier
// ONE thread merges waves 0, 1, ... in order.
template <class T, int kWaves>
__device__ __forceinline__ void wave_store(T (&part)[kWaves], const T& v) {
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
}

template <class T, int kWaves, class Merge>
__device__ __forceinline__ T waves_in_order(const T (&part)[kWaves], Merge merge) {
    T s = part[0];
    for (int w = 1; w < kWaves; ++w) merge(s, part[w]);
    return s;
}

// ... and whole, for a workgroup of kWaves waves with one value per lane: the butterfly, the store, one __syncthreads, the waves in order.
// True in thread 0 alone, whose `v` is then the workgroup's sum.
template <class T, int kWaves, class Merge>
__device__ __forceinline__ bool block_reduce(T& v, T (&part)[kWaves], Merge merge) {
    wave_butterfly(v, merge);
    wave_store(part, v);
    __syncthreads();
    if (threadIdx.x != 0) return false;
    v = waves_in_order(part, merge);
    return true;
}

}  // namespace pp
