"""ctypes binding of tests/csrc/libppenv_playpairshim.so — the paired-statistics arithmetic of the HIP kernels
(isaacgym_amd/csrc/ppenv_play_pair_device.h) compiled for the host, built the way play_shim_binding.lib() builds the accounting's — and a
numpy restatement of include/ppenv_play_pair.h's rule, written from the header's words alone.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd._lib import PlayPairTotals

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "play_pair_shim.cpp")
_HDRS = [os.path.join(_HERE, "csrc", "butterfly_host.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_play_pair_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_play_pair.h"), os.path.join(_HERE, "..", "include", "ppenv_play_group.h"),
         os.path.join(_HERE, "..", "include", "ppenv_play.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_playpairshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        i32, vp = C.c_int32, C.c_void_p
        L.play_pair_shim_sizeof_totals.restype = C.c_size_t
        L.play_pair_shim_reset.restype = L.play_pair_shim_record.restype = L.play_pair_shim_reduce.restype = None
        L.play_pair_shim_reset.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.play_pair_shim_record.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.play_pair_shim_reduce.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp]
        assert L.play_pair_shim_sizeof_totals() == C.sizeof(PlayPairTotals) == 80
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostPairs:
    """isaacgym_amd.play.PairStats in numpy, stepped by the kernel bodies on the CPU."""

    def __init__(self, envs_per_group, groups, num_agents, episodes, baseline):
        self.L = lib()
        self.sizes = S, G, A, M = int(envs_per_group), int(groups), int(num_agents), int(episodes)
        self.baseline = np.ascontiguousarray(np.broadcast_to(np.asarray(baseline, np.int32), (G,)))
        self.cur_reward = np.full(S * G * A, 7.0, np.float32)           # garbage: reset() must clear it
        self.cur_steps = np.full(S * G, 7, np.int32)
        self.count = np.full(S * G, 7, np.int32)
        self.ret = np.full(S * G * M * A, 7.0, np.float32)
        self.len = np.full(S * G * M, 7, np.int32)
        self.out = np.full(G * C.sizeof(PlayPairTotals), 0x55, np.uint8)
        self.reset()

    def reset(self):
        self.L.play_pair_shim_reset(*self.sizes, _p(self.cur_reward), _p(self.cur_steps), _p(self.count), _p(self.ret), _p(self.len))

    def record(self, rew, done):
        r, d = np.ascontiguousarray(rew, np.float32), np.ascontiguousarray(done, np.int64)
        assert r.size == d.size == self.cur_reward.size
        self.L.play_pair_shim_record(_p(r), _p(d), *self.sizes, _p(self.cur_reward), _p(self.cur_steps), _p(self.count), _p(self.ret), _p(self.len))

    def reduce(self, baseline=None):
        b = self.baseline if baseline is None else np.ascontiguousarray(baseline, np.int32)
        self.L.play_pair_shim_reduce(*self.sizes, _p(b), _p(self.count), _p(self.ret), _p(self.len), _p(self.out))
        raw, n = self.out.tobytes(), C.sizeof(PlayPairTotals)
        return [PlayPairTotals.from_buffer_copy(raw[g * n:(g + 1) * n]) for g in range(self.sizes[1])]

    def state_bytes(self):
        """cur_reward, cur_steps, count, ret, len as bytes (PairStats.state_bytes())."""
        return tuple(a.tobytes() for a in (self.cur_reward, self.cur_steps, self.count, self.ret, self.len))


# ---- the rule of include/ppenv_play_pair.h in numpy
def numpy_record(rews, dones, S, G, A, M):
    """[steps, rows] rewards and done words -> (count [G, S] i32, ret [G, S, M, A] f32 with NaN where not played, len [G, S, M] i32)."""
    N = S * G
    cr, steps = np.zeros((N, A), np.float32), np.zeros(N, np.int32)
    count, ret, length = np.zeros(N, np.int32), np.full((N, M, A), np.nan, np.float32), np.zeros((N, M), np.int32)
    for t in range(rews.shape[0]):
        cr = (cr + rews[t].reshape(N, A).astype(np.float32)).astype(np.float32)
        steps = steps + 1
        fin = dones[t].reshape(N, A)[:, 0] != 0
        for e in np.nonzero(fin)[0]:
            if count[e] < M:
                ret[e, count[e]], length[e, count[e]] = cr[e], steps[e]
                count[e] += 1
        cr[fin], steps[fin] = 0.0, 0
    return count.reshape(G, S), ret.reshape(G, S, M, A), length.reshape(G, S, M)


def numpy_reduce(count, ret, length, baseline):
    """-> per cell dict(pairs, steps_diff: ints; diff, diff_sq, cell, base: fp64 [A], np.sum of the fp64 terms; abs_*: the sums of |term|)."""
    G, S, M, A = ret.shape
    out = []
    for g in range(G):
        b = int(np.broadcast_to(np.asarray(baseline), (G,))[g])
        both = np.minimum(count[g], count[b])                            # [S]
        mask = np.arange(M)[None, :] < both[:, None]                     # [S, M]
        x, y = ret[g][mask].astype(np.float64), ret[b][mask].astype(np.float64)     # [n, A]
        d = x - y
        out.append(dict(pairs=int(mask.sum()), steps_diff=int((length[g][mask].astype(np.int64) - length[b][mask].astype(np.int64)).sum()),
                        diff=d.sum(0), diff_sq=(d * d).sum(0), cell=x.sum(0), base=y.sum(0),
                        abs_diff=np.abs(d).sum(0), abs_diff_sq=(d * d).sum(0), abs_cell=np.abs(x).sum(0), abs_base=np.abs(y).sum(0)))
    return out


def check_sums(got, want, num_agents, what=""):
    """A PlayPairTotals (or a PairStats.read() dict) against numpy_reduce's entry: the integers equal; every fp64 sum within
    n x 2^-52 x sum|term| of numpy's — the terms are the same fp64 numbers on both sides, only the order of n - 1 additions differs."""
    get = (lambda k: got[k + "_sum" if k in ("cell", "base") else k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    assert int(get("pairs")) == want["pairs"] and int(get("steps_diff")) == want["steps_diff"], (what, int(get("pairs")), want["pairs"])
    n = max(want["pairs"], 1)
    for k in ("diff", "diff_sq", "cell", "base"):
        for a in range(num_agents):
            bound = n * 2.0 ** -52 * want["abs_" + k][a]
            assert abs(get(k)[a] - want[k][a]) <= bound, (what, k, a, get(k)[a], want[k][a], bound)


# ---- the cases the host and the GPU tests share
STEPS = 40
WORDS = (1, 2, 1 << 32)
#          S    G  A  M  baseline
SHAPES = [(1,   3, 1, 1, 1), (65, 3, 2, 3, 1), (257, 3, 1, 3, 1), (65, 3, 1, 1, [2, 0, 1]), (257, 3, 2, 1, [1, 1, 0]), (1, 3, 2, 3, [0, 2, 2])]


def streams(S, G, A, steps=STEPS, seed=11):
    """[steps, rows] float32 rewards and int64 done words in the style of play_shim_binding's generators (its rewards(); done words 1, 2 and
    2^32 at p = 0.08 per step plus a burst), with — where there are envs enough — env 3 of every group never finishing and env 2 of every
    group finishing every other step (far more than M games)."""
    import play_shim_binding as ps
    N = S * G
    dones = ps.scripted_dones(steps, N, A, words=WORDS, seed=seed)
    if S > 3:
        d = dones.reshape(steps, N, A)
        d[:, 3::S, :] = 0
        d[::2, 2::S, :] = 1 << 32
    return ps.rewards(steps, N * A, seed=seed + 1), dones
