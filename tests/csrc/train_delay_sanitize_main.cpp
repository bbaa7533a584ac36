// train_delay_sanitize_main.cpp — a stand-alone driver of train_delay_shim.cpp (the training delay line's kernel body on the host) over
// one case per width, for a build under -fsanitize=address,undefined: the ring is sized by pp_train_delay_ring_bytes' own arithmetic
// (pp::delay_ring_bytes of hi + 1 slots) and every other buffer exactly as include/ppenv_train_delay.h says, so an index past a row, a
// slot, a table or the ring is reported, and so is signed overflow in the draw.  age, episode and delay start as garbage: reset clears
// the first two, and the first push of every row redraws the third.  TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_train_delay_host.py, never loaded into Python.  Prints one line per case and exits 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "train_delay_shim.cpp"

namespace {

uint32_t rng_state = 12345u;
uint32_t word() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state;
}

// rows x W words, delays drawn in lo .. hi, A agents; `in` has a stride of W + pad_in, `out` one of W + pad_out
int run(int32_t rows, int32_t A, int32_t W, int32_t lo, int32_t hi, int32_t channel, int32_t pad_in, int32_t pad_out) {
    const pp_train_delay_consts c = {lo, hi, 0x9E3779B97F4A7C15ull * (uint64_t)(rows + W), 0x7FFFFFFF - rows, channel};      // the largest env ids
    if (!pp::train_delay_consts_ok(c)) return 1;
    const size_t ring_bytes = pp::delay_ring_bytes(rows, W, hi + 1);
    if (ring_bytes == 0) return 1;
    const int64_t ld_in = W + pad_in, ld_out = W + pad_out;
    std::vector<uint32_t> ring(ring_bytes / sizeof(uint32_t), 0x55555555u), in((size_t)rows * ld_in), out((size_t)rows * ld_out, 0x55555555u);
    std::vector<int32_t> age(rows, 0x55555555), episode(rows, 0x55555555), delay(rows, (int32_t)0xD5555555);
    std::vector<int64_t> done(rows);
    train_delay_shim_reset(rows, age.data(), episode.data());
    const int pushes = 3 * (hi + 1) + 5;
    uint64_t sum = 0;
    for (int t = 0; t < pushes; ++t) {
        for (uint32_t& v : in) v = word();
        for (int32_t e = 0; e < rows / A; ++e) {
            const int64_t w = (word() >> 8) % 5 == 0 ? ((e & 1) ? 2 : (int64_t)1 << 32) : 0;
            for (int32_t a = 0; a < A; ++a) done[(size_t)A * e + a] = w;
        }
        train_delay_shim_push(in.data(), ld_in, t == 0 ? nullptr : done.data(), rows, A, W, &c, delay.data(), age.data(), episode.data(), ring.data(), out.data(),
                              ld_out);
        for (int32_t r = 0; r < rows; ++r) {
            if (delay[r] < lo || delay[r] > hi || episode[r] < 1 || age[r] < 1 || age[r] > t + 1) return 1;
            for (int32_t col = 0; col < W; ++col) sum += out[(size_t)r * ld_out + col];
            for (int64_t col = W; col < ld_out; ++col)                   // the padding of out stays as it was
                if (out[(size_t)r * ld_out + col] != 0x55555555u) return 1;
        }
    }
    std::printf("rows %d A %d W %d delays %d..%d: pushes %d checksum %llu\n", rows, A, W, lo, hi, pushes, (unsigned long long)sum);
    return 0;
}

}  // namespace

int main() {
    int rc = run(130, 2, 1, 0, 15, 0, 0, 0);
    rc |= run(65, 1, 7, 0, 3, 1, 3, 1);
    rc |= run(130, 1, 27, 15, 15, 0, 0, 1);
    rc |= run(64, 2, 80, 1, 1, 1, 3, 0);
    rc |= run(63, 1, 313, 2, 15, 0, 3, 1);
    rc |= run(1, 1, 512, 0, 0, 1, 0, 0);
    return rc;
}
