// packed_pairs_shim.cpp — the two-at-a-time helpers of isaacgym_amd/csrc/ppenv_device.h (f2 / V3p / S3p) next to the scalar helpers
// they stand for, compiled for the host with -ffp-contract=off so that every operation rounds on its own.  TEST INFRASTRUCTURE ONLY
// (tests/test_packed_pairs_host.py): "the arithmetic per element is the scalar code's" means bit equality here.
//
// pk_shim_eval(op, n, in, packed, scalar): row r reads kIn floats at in + r * kIn and writes kOut floats to packed + r * kOut (the packed
// helper: low halves first, then high halves) and to scalar + r * kOut (the scalar helper applied to the low and to the high operands).
// Returns the number of floats per row that the op defines (the rest stay untouched), or -1 for an unknown op.
#include "../../isaacgym_amd/csrc/ppenv_device.h"

using namespace pp;

namespace {
constexpr int kIn = 32, kOut = 12;

M3 m3(const float* p) { return ldm(p); }
S3 s3(const float* p) { S3 s = {p[0], p[1], p[2], p[3], p[4], p[5]}; return s; }
void put(float* o, V3 a, V3 b) { o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = b.x; o[4] = b.y; o[5] = b.z; }
void put(float* o, S3 a, S3 b) {
    const float v[12] = {a.xx, a.yy, a.zz, a.xy, a.xz, a.yz, b.xx, b.yy, b.zz, b.xy, b.xz, b.yz};
    for (int k = 0; k < 12; k++) o[k] = v[k];
}
}  // namespace

extern "C" {

int pk_shim_in_floats(void) { return kIn; }
int pk_shim_out_floats(void) { return kOut; }

int pk_shim_eval(int op, int n, const float* in, float* packed, float* scalar) {
    int used = -1;
    for (int r = 0; r < n; r++) {
        const float* p = in + (size_t)r * kIn;
        float* P = packed + (size_t)r * kOut;
        float* Q = scalar + (size_t)r * kOut;
        const M3 E = m3(p);                                   // p[0:9]
        const V3 a = ld3(p + 9), b = ld3(p + 12), c = ld3(p + 15), d = ld3(p + 18);
        const S3 sa = s3(p + 9), sb = s3(p + 15);             // (the symmetric operands overlay the vectors: an op uses one or the other)
        const float k = p[21];
        switch (op) {
        case 0: { S3p x = rot_sym(E, pk(sa, sb)); put(P, lo(x), hi(x)); put(Q, rot_sym(E, sa), rot_sym(E, sb)); used = 12; break; }
        case 1: { V3p x = mul(E, pk(a, b)); put(P, lo(x), hi(x)); put(Q, mul(E, a), mul(E, b)); used = 6; break; }
        case 2: { V3p x = tmul(E, pk(a, b)); put(P, lo(x), hi(x)); put(Q, tmul(E, a), tmul(E, b)); used = 6; break; }
        case 3: { V3p x = cross(c, pk(a, b)); put(P, lo(x), hi(x)); put(Q, cross(c, a), cross(c, b)); used = 6; break; }
        case 4: { V3p x = cross(pk(a, b), c); put(P, lo(x), hi(x)); put(Q, cross(a, c), cross(b, c)); used = 6; break; }
        case 5: { f2 x = dot(c, pk(a, b)); P[0] = x[0]; P[1] = x[1]; Q[0] = dot(c, a); Q[1] = dot(c, b); used = 2; break; }
        case 6: { f2 x = dot(pk(a, b), pk(c, d)); P[0] = x[0]; P[1] = x[1]; Q[0] = dot(a, c); Q[1] = dot(b, d); used = 2; break; }
        case 7: {
            const V3 u = ld3(p), v = ld3(p + 3);
            S3p x = pk(sa, sb); sym_rank1_sub(x, pk(u, v), k);
            S3 ya = sa, yb = sb; sym_rank1_sub(ya, u, k); sym_rank1_sub(yb, v, k);
            put(P, lo(x), hi(x)); put(Q, ya, yb); used = 12; break;
        }
        case 8: {
            const V3 u = ld3(p), v = ld3(p + 3);
            V3p x = mul(pk(sa, sb), pk(u, v)); put(P, lo(x), hi(x)); put(Q, mul(sa, u), mul(sb, v)); used = 6; break;
        }
        case 9: { V3p x = heading_rotate(p + 22, pk(a, b)); put(P, lo(x), hi(x)); put(Q, heading_rotate(p + 22, a), heading_rotate(p + 22, b)); used = 6; break; }
        case 10: { V3p x = pk(a, b) + pk(c, d) * k; put(P, lo(x), hi(x)); put(Q, a + c * k, b + d * k); used = 6; break; }
        default: return -1;
        }
    }
    return used;
}

}  // extern "C"
