"""ctypes binding of tests/csrc/libppenv_pkshim.so — the two-at-a-time helpers of isaacgym_amd/csrc/ppenv_device.h (f2 / V3p / S3p)
beside their scalar counterparts, compiled for the host with -ffp-contract=off (every operation rounds on its own), built the way
shim_binding.lib() builds the step's.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "packed_pairs_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_model_g1.h"),
         os.path.join(_HERE, "..", "include", "ppenv.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_pkshim.so")
_lib = None

# op index of pk_shim_eval -> (name, what the packed helper is compared with)
OPS = {0: ("rot_sym", "E S E^T of (S_lo, S_hi)"), 1: ("mul", "E v of (v_lo, v_hi)"), 2: ("tmul", "E^T v of (v_lo, v_hi)"),
       3: ("cross(V3, V3p)", "c x v of (v_lo, v_hi)"), 4: ("cross(V3p, V3)", "v x c of (v_lo, v_hi)"), 5: ("dot(V3, V3p)", "c . v of (v_lo, v_hi)"),
       6: ("dot(V3p, V3p)", "element by element"), 7: ("sym_rank1_sub", "S -= u u^T k of (S_lo, u_lo), (S_hi, u_hi)"),
       8: ("mul(S3p, V3p)", "element by element"), 9: ("heading_rotate", "the observation row's body block"), 10: ("operator+ / operator*", "a + c k")}


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        L.pk_shim_in_floats.restype = L.pk_shim_out_floats.restype = L.pk_shim_eval.restype = C.c_int
        L.pk_shim_eval.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def evaluate(op, operands):
    """operands [n, pk_shim_in_floats()] fp32 -> (packed [n, used], scalar [n, used]) as uint32 bit patterns."""
    L = lib()
    x = np.ascontiguousarray(operands, np.float32)
    n = x.shape[0]
    assert x.shape == (n, L.pk_shim_in_floats())
    packed, scalar = (np.full((n, L.pk_shim_out_floats()), np.nan, np.float32) for _ in range(2))
    used = L.pk_shim_eval(op, n, x.ctypes.data, packed.ctypes.data, scalar.ctypes.data)
    assert used > 0, f"pk_shim_eval: unknown op {op}"
    return packed[:, :used].view(np.uint32), scalar[:, :used].view(np.uint32)
