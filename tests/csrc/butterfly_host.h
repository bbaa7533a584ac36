// butterfly_host.h — the accounting kernels' summation order walked on a plain array of lanes, for the host builds of the shims: the xor
// butterfly of every wave of 64 lanes (stage by stage, each lane adding its partner's value of before the stage; strides 32 down to 1 or 1
// up to 32, as the kernel under test states), then the waves in order.  TEST INFRASTRUCTURE ONLY.  Written from the words of include/*.h,
// apart from the device code (isaacgym_amd/csrc/ppenv_reduce_device.h): the partner here is always lane l ^ off itself.
#pragma once
#include <vector>

namespace butterfly {

enum order { descending, ascending };

// lane[0 .. n), n a multiple of 64: afterwards every lane of a wave holds the wave's sum, and the waves' sums merged in order are returned.
template <class T, class Merge>
T block_sum(T* lane, int n, order o, Merge merge) {
    std::vector<T> next(n);
    for (int stage = 0; stage < 6; ++stage) {
        const int off = o == ascending ? 1 << stage : 32 >> stage;
        for (int l = 0; l < n; ++l) {
            next[l] = lane[l];
            merge(next[l], lane[l ^ off]);
        }
        for (int l = 0; l < n; ++l) lane[l] = next[l];
    }
    T s = lane[0];
    for (int w = 1; w < n / 64; ++w) merge(s, lane[64 * w]);
    return s;
}

}  // namespace butterfly
