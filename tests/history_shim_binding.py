"""ctypes binding of tests/csrc/libppenv_historyshim.so — the observation and action history of the HIP kernel
(isaacgym_amd/csrc/ppenv_history_device.h) compiled for the host and walked in the kernel's order, built the way
train_delay_shim_binding.lib() builds the delay line's — and the case generator the host and GPU tests of the history share.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "history_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", name) for name in ("ppenv_history_device.h", "ppenv_device.h")] + \
        [os.path.join(_HERE, "..", "include", name) for name in ("ppenv_history.h", "ppenv.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_historyshim.so")
_lib = None
OBS, PREV, ACT, ZERO = range(4)             # pp::HISTORY_*
SHAPES = ((80, 7), (313, 27))               # (n, A): the 7-dof and the 27-dof task
HISTORIES = ((1, 0), (0, 1), (2, 3), (8, 8))
CANARY = np.float32(-77.25)


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, [])
        i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
        L.history_shim_width.restype = L.history_shim_rows_per_block.restype = i32
        L.history_shim_width.argtypes = [i32] * 4
        L.history_shim_rows_per_block.argtypes = [i32]
        L.history_shim_source.restype = L.history_shim_push.restype = None
        L.history_shim_source.argtypes = [i32] * 6 + [vp]
        L.history_shim_push.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, f32, f32]
        _lib = L
    return _lib


def shim_source(n, A, Ho, Ha, start, c):
    out = np.zeros(3, np.int32)
    lib().history_shim_source(n, A, Ho, Ha, int(start), c, out.ctypes.data_as(C.c_void_p))
    return tuple(int(x) for x in out)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def phased(shape, phase, fill=0.0):
    """A C-contiguous float32 array of `shape` whose first element lies `phase` words past a 16-byte boundary."""
    size = int(np.prod(shape))
    raw = np.empty(size + 8, np.float32)
    at = (-(raw.ctypes.data // 4) % 4 + phase) % 4
    out = raw[at:at + size].reshape(shape)
    out[...] = fill
    assert (out.ctypes.data // 4) % 4 == phase
    return out


def shim_push(obs, act, done, prev, out, num_agents, n, A, Ho, Ha, lo=-1.0, hi=1.0):
    """The kernel body on host arrays: 2-d float32 with unit inner stride (views of wider arrays allowed); writes out[:, :W]."""
    ld = lambda a: 0 if a is None else a.strides[0] // 4
    for a in (obs, act, prev, out):
        assert a is None or (a.dtype == np.float32 and a.strides[1] == 4)
    d = None if done is None else np.ascontiguousarray(done, np.int64)
    lib().history_shim_push(_p(obs), ld(obs), _p(act), ld(act), _p(d), _p(prev), ld(prev), _p(out), ld(out), obs.shape[0], num_agents, n, A, Ho, Ha, lo, hi)
    return out


def case_stream(rows, num_agents, n, A, pushes=6, seed=5):
    """-> obs float32 [T, rows, n], act float32 [T, rows, A], dones int64 [T, rows].  The observations hold NaNs (two payloads), -0.0 and
    infinities; the actions reach beyond [-1, 1] and hold NaN and -0.0.  Agent 0's done word is set (1, 2 or 2^32) on about a quarter of the
    env-steps and copied to the env's other row; where it is not set, agent 1's own word is sometimes set, which the rule ignores."""
    rng = np.random.default_rng(seed + 11 * rows + 1000 * n + num_agents)
    obs = rng.standard_normal((pushes, rows, n)).astype(np.float32)
    act = (1.5 * rng.standard_normal((pushes, rows, A))).astype(np.float32)
    ob, ab = obs.view(np.uint32), act.view(np.uint32)
    pick = rng.random(obs.shape)
    ob[pick < 0.02] = 0x7FC00001
    ob[(pick >= 0.02) & (pick < 0.04)] = 0xFFA12345
    ob[(pick >= 0.04) & (pick < 0.06)] = 0x80000000
    ob[(pick >= 0.06) & (pick < 0.07)] = 0x7F800000
    pick = rng.random(act.shape)
    ab[pick < 0.05] = 0x7FC00000
    ab[(pick >= 0.05) & (pick < 0.1)] = 0x80000000
    ob[0, 0, 0], ob[0, 0, n - 1], ob[1, 0, 0] = 0x7FC00001, 0x80000000, 0xFFA12345         # whatever the draws: one of each in the smallest case too
    ab[0, 0, 0], ab[1, 0, 0], act[2, 0, 0], act[1, 0, A - 1] = 0x7FC00000, 0x80000000, 3.0, -2.5
    N = rows // num_agents
    words = np.array([1, 2, 1 << 32], np.int64)
    env = np.where(rng.random((pushes, N)) < 0.25, words[rng.integers(0, 3, (pushes, N))], 0)
    env[min(2, pushes - 1), 0] = 1 << 32                     # at least one done whose low 32 bits are zero
    dones = np.repeat(env, num_agents, axis=1)
    if num_agents == 2:
        stray = (rng.random((pushes, N)) < 0.3) & (env == 0)
        dones[:, 1::2][stray] = 1
        if N > 1:
            env_free = env[min(3, pushes - 1), 1] == 0
            if env_free:
                dones[min(3, pushes - 1), 3] = 1             # agent 1 alone: no start
    return obs, act, dones
