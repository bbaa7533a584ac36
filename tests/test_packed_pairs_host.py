"""The packed-pair helpers the 7-dof step kernels use (isaacgym_amd/csrc/ppenv_device.h: f2 / V3p / S3p) against the scalar helper applied
to each half: random operands, a host build with -ffp-contract=off, BIT equality.  This pins the header's claim that a pair written as a
2-vector is the scalar code's arithmetic per element: same operations, same order, same roundings."""
import numpy as np
import pytest

import packed_pairs_shim_binding as pk

N = 4096


def operands(seed, scale):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, pk.lib().pk_shim_in_floats())) * scale).astype(np.float32)
    # a share of exact zeros, ones and sign flips: the products whose rounding is trivial must still pair up the same way
    x[rng.random(x.shape) < 0.05] = 0.0
    x[rng.random(x.shape) < 0.02] = 1.0
    return x


@pytest.mark.parametrize("op", sorted(pk.OPS), ids=[pk.OPS[k][0] for k in sorted(pk.OPS)])
@pytest.mark.parametrize("scale", [1.0, 1e-3, 37.0])
def test_packed_helper_is_the_scalar_helper_on_each_half(op, scale):
    packed, scalar = pk.evaluate(op, operands(100 + op, scale))
    assert np.isfinite(scalar.view(np.float32)).all()
    bad = np.argwhere(packed != scalar)
    assert bad.size == 0, (f"{pk.OPS[op][0]} ({pk.OPS[op][1]}): {len(bad)} of {packed.size} outputs differ in their bits, first at row {bad[0][0]} "
                           f"output {bad[0][1]}: packed {packed.view(np.float32)[tuple(bad[0])]!r} scalar {scalar.view(np.float32)[tuple(bad[0])]!r}")


def test_the_halves_do_not_mix():
    """Changing only the high operands leaves every low result as it was, and the other way round."""
    L = pk.lib()
    base = operands(7, 1.0)
    for op in sorted(pk.OPS):
        p0, _ = pk.evaluate(op, base)
        half = p0.shape[1] // 2
        hi_cols = {0: slice(15, 21), 7: slice(3, 6), 8: slice(3, 6)}.get(op, slice(12, 15))       # an operand only the high half reads
        x = base.copy()
        x[:, hi_cols] += 1.0
        if op in (7, 8):
            x[:, 15:21] += 1.0
        p1, _ = pk.evaluate(op, x)
        assert np.array_equal(p0[:, :half], p1[:, :half]), pk.OPS[op][0]
        assert (p0[:, half:] != p1[:, half:]).any(), pk.OPS[op][0]
    assert L.pk_shim_eval(99, 1, base.ctypes.data, base.ctypes.data, base.ctypes.data) == -1
