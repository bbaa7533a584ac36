"""ctypes binding of tests/csrc/libppenv_playdelayshim.so — the control-latency delay line of the HIP kernel
(isaacgym_amd/csrc/ppenv_play_delay_device.h) compiled for the host and walked in the kernel's order, built the way
play_act_shim_binding.lib() builds the actuator accounting's — and a numpy restatement of include/ppenv_play_delay.h's rule, written from the
header's words alone (no ring, no modulo: every pushed array is kept).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import itertools
import os

import numpy as np

from helpers import build_shim

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "play_delay_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_play_delay_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_play_delay.h"), os.path.join(_HERE, "..", "include", "ppenv_play_group.h"),
         os.path.join(_HERE, "..", "include", "ppenv_play.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_playdelayshim.so")
_lib = None
DELAY_MAX, MAX_WIDTH = 15, 512              # PP_PLAY_DELAY_MAX, PP_PLAY_DELAY_MAX_WIDTH
GARBAGE = 0x55555555


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, [])
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.play_delay_shim_rows_per_block.restype = i32
        L.play_delay_shim_rows_per_block.argtypes = [i32]
        L.play_delay_shim_reset.restype = L.play_delay_shim_push.restype = None
        L.play_delay_shim_reset.argtypes = [i32, vp]
        L.play_delay_shim_push.argtypes = [vp, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostDelay:
    """isaacgym_amd.play.Delay in numpy, stepped by the kernel body on the CPU.  Words are uint32; `out` is [rows, ld_out], garbage outside
    the first `width` columns, and stays so."""

    def __init__(self, rows, width, delays, num_agents=1, ld_out=None):
        self.L = lib()
        self.rows, self.width, self.A = int(rows), int(width), int(num_agents)
        self.delay = np.ascontiguousarray(delays, np.int32)
        assert self.delay.shape == (self.rows,) and self.delay.min() >= 0
        self.depth = int(self.delay.max()) + 1
        self.ld_out = self.width if ld_out is None else int(ld_out)
        self.age = np.full(self.rows, GARBAGE, np.int32)                                  # garbage: reset() must clear it
        self.ring = np.full((self.depth, self.rows, self.width), GARBAGE, np.uint32)      # ... and nothing may read this
        self.out = np.full((self.rows, self.ld_out), GARBAGE, np.uint32)
        self.reset()

    def reset(self):
        self.L.play_delay_shim_reset(self.rows, _p(self.age))

    def push(self, x, done=None):
        """x: uint32 [rows, ld_in >= width], C-contiguous; done: int64 [rows] or None.  -> the [rows, width] view of out."""
        assert x.dtype == np.uint32 and x.flags.c_contiguous and x.shape[0] == self.rows and x.shape[1] >= self.width
        d = None if done is None else np.ascontiguousarray(done, np.int64)
        assert d is None or d.shape == (self.rows,)
        self.L.play_delay_shim_push(_p(x), x.shape[1], None if d is None else _p(d), self.rows, self.A, self.width, self.depth, _p(self.delay), _p(self.age),
                                    _p(self.ring), _p(self.out), self.ld_out)
        return self.out[:, :self.width]


# ---- the rule of include/ppenv_play_delay.h in numpy
class NumpyDelay:
    """Every pushed sample is kept (a list of copies); per row the index of the push that began its running episode.  The output of push t
    for row r is the sample of push start[r] + max(t - start[r] - d[r], 0)."""

    def __init__(self, rows, width, delays, num_agents=1):
        self.rows, self.width, self.A = int(rows), int(width), int(num_agents)
        self.d = np.asarray(delays, np.int64)
        self.reset()

    def reset(self):
        self.kept, self.start = [], np.zeros(self.rows, np.int64)

    def push(self, x, done=None):
        t = len(self.kept)
        self.kept.append(np.array(x[:, :self.width], copy=True))
        if done is not None:
            first = np.repeat(np.asarray(done).reshape(-1, self.A)[:, 0] != 0, self.A)     # agent 0's word, for every row of the env
            self.start[first] = t
        src = self.start + np.maximum(t - self.start - self.d, 0)
        out = np.empty((self.rows, self.width), x.dtype)
        for r in range(self.rows):
            out[r] = self.kept[src[r]][r]
        return out


# ---- the cases the host and the GPU tests share
ROWS = (1, 63, 64, 65, 130)
WIDTHS = (1, 7, 27, 80, 313)
DEPTHS = (1, 2, 4, 16)
# (rows, A): every row count with one agent; with two, the counts that are whole envs and every count taken as ENVS (rows = 2 x)
SHAPES = [(r, 1) for r in ROWS] + sorted({(r, 2) for r in ROWS if r % 2 == 0} | {(2 * r, 2) for r in ROWS})
SPECIAL = np.array([0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800000, 0x00000000, 0x00000001], np.uint32)   # -0.0, NaNs with payloads, -inf


def shape_id(shape):
    return f"rows{shape[0]}-A{shape[1]}"


def subcases():
    """(W, depth, pad): pad 1 gives `in` a stride of W + 3 and `out` one of W + 1."""
    return list(itertools.product(WIDTHS, DEPTHS, (0, 1)))


def pushes_of(depth):
    return 3 * depth + 5


def case_delays(rows, depth, seed=5):
    """Mixed per-row delays in 0 .. depth - 1, with depth - 1 on row 0 and (two rows or more) 0 on the last row."""
    d = np.random.default_rng(seed + 31 * rows + depth).integers(0, depth, rows).astype(np.int32)
    d[-1] = 0
    d[0] = depth - 1
    return d


def case_stream(rows, A, W, depth, pad, seed=11):
    """-> xs uint32 [T, rows, W + 3 * pad] (random words: one in 256 is a NaN pattern as it is; one in 8 replaced by SPECIAL words) and
    dones int64 [T, rows] with T = 3 * depth + 5: random words 1, 2 and 2^32 on one env-step in five — the rows of an env share agent 0's
    word, EXCEPT that agent 1's own word is set where agent 0's is not on some steps, which the rule ignores; env 0 is done on the very
    first push, and the last env on the consecutive pushes 3 and 4 (and 0 again where it is env 0)."""
    T = pushes_of(depth)
    rng = np.random.default_rng(seed + 7 * rows + 1000 * W + 100000 * depth + pad)
    xs = rng.integers(0, 2 ** 32, (T, rows, W + 3 * pad), dtype=np.uint64).astype(np.uint32)
    sp = rng.random(xs.shape) < 0.125
    xs[sp] = SPECIAL[rng.integers(0, len(SPECIAL), int(sp.sum()))]
    xs.reshape(-1)[:len(SPECIAL)] = SPECIAL                        # the smallest streams carry them too (word 0, -0.0, and word 4, a NaN, lie in column 0 of any stride used)
    N = rows // A
    words = np.array([1, 2, 1 << 32], np.int64)
    env = np.where(rng.random((T, N)) < 0.2, words[rng.integers(0, 3, (T, N))], 0)
    env[0, 0] = 1 << 32
    env[3:5, N - 1] = 2
    dones = np.repeat(env, A, axis=1)
    if A == 2:
        stray = (rng.random((T, N)) < 0.3) & (env == 0)
        dones[:, 1::2][stray] = 1
    return xs, dones
