// play_delay_sanitize_main.cpp — a stand-alone driver of play_delay_shim.cpp (the delay line's kernel body on the host) over one case
// per width, for a build under -fsanitize=address,undefined: the ring is sized by pp_play_delay_ring_bytes' own arithmetic
// (pp::delay_ring_bytes) and every other buffer exactly as include/ppenv_play_delay.h says, so an index past a row, a slot or the ring
// is reported.  TEST INFRASTRUCTURE ONLY; built and run by tests/test_play_delay_host.py, never loaded into Python.  Prints one line
// per case and exits 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "play_delay_shim.cpp"

namespace {

uint32_t rng_state = 12345u;
uint32_t word() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state;
}

// rows x W words, `depth` slots, A agents; `in` has a stride of W + pad_in, `out` one of W + pad_out
int run(int32_t rows, int32_t A, int32_t W, int32_t depth, int32_t pad_in, int32_t pad_out) {
    const size_t ring_bytes = pp::delay_ring_bytes(rows, W, depth);
    if (ring_bytes == 0) return 1;
    const int64_t ld_in = W + pad_in, ld_out = W + pad_out;
    std::vector<uint32_t> ring(ring_bytes / sizeof(uint32_t), 0x55555555u), in((size_t)rows * ld_in), out((size_t)rows * ld_out, 0x55555555u);
    std::vector<int32_t> age(rows, 0x55555555), delay(rows);
    std::vector<int64_t> done(rows);
    for (int32_t r = 0; r < rows; ++r) delay[r] = (int32_t)(word() >> 8) % depth;
    delay[0] = depth - 1;
    delay[rows - 1] = 0;
    play_delay_shim_reset(rows, age.data());
    const int pushes = 3 * depth + 5;
    uint64_t sum = 0;
    for (int t = 0; t < pushes; ++t) {
        for (uint32_t& v : in) v = word();
        for (int32_t e = 0; e < rows / A; ++e) {
            const int64_t w = (word() >> 8) % 5 == 0 ? ((e & 1) ? 2 : (int64_t)1 << 32) : 0;
            for (int32_t a = 0; a < A; ++a) done[(size_t)A * e + a] = w;
        }
        play_delay_shim_push(in.data(), ld_in, t == 0 ? nullptr : done.data(), rows, A, W, depth, delay.data(), age.data(), ring.data(), out.data(), ld_out);
        for (int32_t r = 0; r < rows; ++r)
            for (int32_t c = 0; c < W; ++c) sum += out[(size_t)r * ld_out + c];
        for (int32_t r = 0; r < rows; ++r)                              // the padding of out stays as it was
            for (int64_t c = W; c < ld_out; ++c)
                if (out[(size_t)r * ld_out + c] != 0x55555555u) return 1;
    }
    std::printf("rows %d A %d W %d depth %d: pushes %d checksum %llu\n", rows, A, W, depth, pushes, (unsigned long long)sum);
    return 0;
}

}  // namespace

int main() {
    int rc = run(130, 2, 1, 16, 0, 0);
    rc |= run(65, 1, 7, 4, 3, 1);
    rc |= run(130, 1, 27, 16, 0, 1);
    rc |= run(64, 2, 80, 2, 3, 0);
    rc |= run(63, 1, 313, 16, 3, 1);
    rc |= run(1, 1, 512, 1, 0, 0);
    return rc;
}
