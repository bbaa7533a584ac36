"""ctypes binding of tests/csrc/libppenv_servecurricshim.so — the serve-curriculum arithmetic of the HIP kernels
(isaacgym_amd/csrc/ppenv_serve_curric_device.h) compiled for the host, built the way serve_shim_binding.lib() builds the plan's — and
`NumpyCurric`, the rule of include/ppenv_serve_curric.h restated in numpy from the header's words (the linear count over the table where
the device header bisects; test_serve_plan_host.np_serve for the ball).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd import _lib, serve
from serve_shim_binding import DEFAULTS

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "serve_curric_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", n) for n in ("ppenv_serve_curric_device.h", "ppenv_serve_device.h", "ppenv_device.h")] + \
        [os.path.join(_HERE, "..", "include", n) for n in ("ppenv_serve_curric.h", "ppenv_serve.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_servecurricshim.so")
_shim = None

U32, F32, F64, I64 = np.uint32, np.float32, np.float64, np.int64
ONE = 1 << 24
DROPPED = -2 ** 63
CHUNK = 16384


def lib():
    global _shim
    if _shim is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        i32, i64, u32, u64, vp, f32 = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_float
        cp, sp = C.POINTER(_lib.ServeCurric), C.POINTER(_lib.ServeCurricState)
        for name in ("layout", "consts", "fill", "step", "fold", "update"):
            getattr(L, f"curric_shim_{name}").restype = None
        L.curric_shim_layout.argtypes = L.curric_shim_consts.argtypes = [vp]
        L.curric_shim_invalid.argtypes = [cp, C.POINTER(_lib.ServeCell)]
        L.curric_shim_u24.restype, L.curric_shim_u24.argtypes = u32, [u64, u32, u32]
        L.curric_shim_uniform.restype, L.curric_shim_uniform.argtypes = f32, [u64, u32, u32]
        L.curric_shim_bin.restype, L.curric_shim_bin.argtypes = i32, [vp, i32, u32]
        L.curric_shim_q.restype, L.curric_shim_q.argtypes = i64, [f32]
        L.curric_shim_fill.argtypes = [cp, i32, sp, vp]
        L.curric_shim_step.argtypes = [cp, vp, vp, sp, vp, vp, vp]
        L.curric_shim_fold.argtypes = [vp, vp, i64, i32, vp]
        L.curric_shim_update.argtypes = [cp, i32, vp, sp]
        _shim = L
    return _shim


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_curric(num_envs, bins, form, layout, reset_rows=1, num_agents=1, seed=0, env_id_offset=0, power=1, mix=0.25, alpha=0.3, n_bins=None):
    """(pp_serve_curric pointing at host cells, the cells array, the resolved cells) as curriculum.ServeCurriculum builds them; n_bins: an override, for the refusals."""
    resolved = serve.resolve_cells(bins, DEFAULTS, serve.AXES_27DOF)
    arr = serve.cell_structs(resolved)
    cur = _lib.ServeCurric(num_envs=num_envs, env_id_offset=env_id_offset, seed=seed & 0xFFFFFFFFFFFFFFFF, form=form, layout=layout, reset_rows=reset_rows,
                           num_agents=num_agents, bins=len(resolved) if n_bins is None else n_bins, power=power, mix=mix, alpha=alpha, cells=C.cast(arr, C.c_void_p))
    return cur, arr, resolved


class _State:
    """The state arrays both restatements keep, and their comparison."""
    NAMES = ("count", "next_bin", "cur_bin", "ret", "games", "mean", "dropped", "cdf")

    def _alloc(self, n, B, layout):
        self.count, self.next_bin, self.cur_bin, self.ret = np.zeros(n, U32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, F32)
        self.games, self.mean, self.dropped, self.cdf = np.zeros(B, I64), np.zeros(B, F32), np.zeros(B, I64), np.zeros(B, U32)
        self.out = np.zeros((3, n) if layout == _lib.SERVE_LAYOUT_SOA3 else (n, 5), F32)

    def words(self):
        """{name: the array's words as integers} of every state array and the buffer."""
        return {k: np.ascontiguousarray(getattr(self, k)).view(U32 if getattr(self, k).dtype.itemsize == 4 else np.uint64).copy() for k in self.NAMES + ("out",)}

    def prob(self):
        return np.diff(self.cdf.astype(I64), prepend=0) / float(ONE)


def same_words(a, b):
    """The names whose words differ between two words() dicts."""
    return [k for k in a if not np.array_equal(a[k], b[k])]


class HostCurric(_State):
    """curriculum.ServeCurriculum in numpy, stepped by the kernel bodies on the CPU."""

    def __init__(self, num_envs, bins, form, layout, reset_rows=1, num_agents=1, seed=0, env_id_offset=0, power=1, mix=0.25, alpha=0.3):
        self.L = lib()
        n = self.num_envs = int(num_envs)
        self.cur, self._cells, self.cells = host_curric(n, bins, form, layout, reset_rows, num_agents, seed, env_id_offset, power, mix, alpha)
        assert self.L.curric_shim_invalid(C.byref(self.cur), self._cells) == 0
        self.bins, self.reset_rows, self.num_agents = len(self.cells), reset_rows, num_agents
        self._alloc(n, self.bins, layout)
        self.state = _lib.ServeCurricState(*(getattr(self, k).ctypes.data for k in self.NAMES))
        self.fill()

    def fill(self):
        self.L.curric_shim_fill(C.byref(self.cur), self.bins, C.byref(self.state), _p(self.out))

    def step(self, rew, reset, fin_bin_t, fin_q_t):
        """fin_bin_t [N] int32 / fin_q_t [N] int64: the caller's rows, written in place."""
        rew, reset = np.ascontiguousarray(rew, F32), np.ascontiguousarray(reset, I64)
        assert rew.size == self.num_agents * self.num_envs and reset.size == self.reset_rows * self.num_envs
        assert fin_bin_t.dtype == np.int32 and fin_q_t.dtype == I64 and fin_bin_t.flags.c_contiguous and fin_q_t.flags.c_contiguous
        self.L.curric_shim_step(C.byref(self.cur), _p(rew), _p(reset), C.byref(self.state), _p(self.out), _p(fin_bin_t), _p(fin_q_t))

    def fold(self, fin_bin, fin_q):
        fin_bin, fin_q = np.ascontiguousarray(fin_bin, np.int32), np.ascontiguousarray(fin_q, I64)
        tot = np.zeros((3, self.bins), I64)
        self.L.curric_shim_fold(_p(fin_bin), _p(fin_q), fin_bin.size, self.bins, _p(tot))
        return tot

    def update(self, tot):
        tot = np.ascontiguousarray(tot, I64)
        self.L.curric_shim_update(C.byref(self.cur), self.bins, _p(tot), C.byref(self.state))


def np_q(x):
    """q of float32 values: the truncating cast of x * 65536 in double; a non-finite or beyond-2^31 return is DROPPED."""
    x = np.asarray(x, F32)
    bad = ~np.isfinite(x) | (np.abs(x) > F32(2147483648.0))
    q = np.trunc(np.where(bad, F32(0), x).astype(F64) * 65536.0).astype(I64)
    return np.where(bad, I64(DROPPED), q)


class NumpyCurric(_State):
    """The rule in numpy, from the words of include/ppenv_serve_curric.h."""

    def __init__(self, num_envs, bins, form, layout, reset_rows=1, num_agents=1, seed=0, env_id_offset=0, power=1, mix=0.25, alpha=0.3, defaults=DEFAULTS,
                 axes=serve.AXES_27DOF):
        n = self.num_envs = int(num_envs)
        self.cells = serve.resolve_cells(bins, defaults, axes)
        self.full = [dict(DEFAULTS, **c) for c in self.cells]              # np_serve reads every axis; the layout decides which it uses
        self.bins, self.form, self.layout, self.reset_rows, self.num_agents = len(self.cells), form, layout, reset_rows, num_agents
        self.seed, self.off, self.power, self.mix, self.alpha = seed & 0xFFFFFFFFFFFFFFFF, env_id_offset, int(power), F32(mix), F32(alpha)
        self._alloc(n, self.bins, layout)
        self.fill()

    def bin_of(self, e, j):
        from test_serve_plan_host import ubits
        u24 = ubits(self.seed, (self.off + np.asarray(e)).astype(U32), np.asarray(j, U32), 5)
        return (self.cdf[None, :self.bins - 1] <= u24[:, None]).sum(1).astype(np.int32)

    def serve(self, e, j, bins):
        """serve(e, j) drawn from cells[bins]: rows [len(e), 3] or [len(e), 5]."""
        from test_serve_plan_host import np_serve
        e = np.asarray(e)
        if e.size == 0:
            return np.zeros((0, 3 if self.layout == _lib.SERVE_LAYOUT_SOA3 else 5), F32)
        # np_serve draws group g = env // S with key = offset + env: one env at a time would be slow, so every env is a group of one ...
        n = int(e.max()) + 1
        resolved = [self.full[0]] * n
        count = np.zeros(n, U32)
        for env, b, jj in zip(e.tolist(), np.asarray(bins).tolist(), np.asarray(j).tolist()):
            resolved[env], count[env] = self.full[b], jj
        out = np_serve(resolved, n, self.form, self.layout, self.seed, self.off, False, count)
        return out[:, e].T if self.layout == _lib.SERVE_LAYOUT_SOA3 else out[e]

    def _store(self, e, rows):
        if self.layout == _lib.SERVE_LAYOUT_SOA3:
            self.out[:, e] = rows.T
        else:
            self.out[e] = rows

    def fill(self):
        B, e = self.bins, np.arange(self.num_envs)
        self.cdf[:] = [((b + 1) << 24) // B for b in range(B)]
        self.next_bin[:] = self.bin_of(e, self.count)
        self._store(e, self.serve(e, self.count, self.next_bin))
        self.cur_bin[:] = -1
        self.ret[:] = 0

    def step(self, rew, reset, fin_bin_t, fin_q_t):
        rew, reset = np.asarray(rew, F32).ravel(), np.asarray(reset, I64).ravel()
        self.ret = (self.ret + rew[::self.num_agents]).astype(F32)
        fired = reset[::self.reset_rows] != 0
        fin_bin_t[:] = np.where(fired, self.cur_bin, -1)
        fin_q_t[fired] = np_q(self.ret[fired])
        self.ret[fired] = 0
        self.cur_bin[fired] = self.next_bin[fired]
        self.count[fired] += 1
        e = np.nonzero(fired)[0]
        self.next_bin[e] = self.bin_of(e, self.count[e])
        self._store(e, self.serve(e, self.count[e], self.next_bin[e]))

    def fold(self, fin_bin, fin_q):
        fin_bin, fin_q = np.asarray(fin_bin).ravel(), np.asarray(fin_q, I64).ravel()
        tot = np.zeros((3, self.bins), I64)
        live = fin_bin >= 0
        drop = live & (fin_q == DROPPED)
        good = live & ~drop
        np.add.at(tot[0], fin_bin[good], 1)
        np.add.at(tot[1], fin_bin[good], fin_q[good])
        np.add.at(tot[2], fin_bin[drop], 1)
        return tot

    def update(self, tot):
        B = self.bins
        for b in range(B):
            n, q, d = (int(tot[k][b]) for k in range(3))
            if n > 0:
                m = F32(F64(q) / (F64(65536.0) * F64(n)))
                self.mean[b] = m if self.games[b] == 0 else F32(self.mean[b] + F32(self.alpha * F32(m - self.mean[b])))
                self.games[b] += n
            self.dropped[b] += d
        seen, idx = self.games > 0, np.arange(B)
        w = []
        for b in range(B):
            rank = 1 + int((seen & ((self.mean < self.mean[b]) | ((self.mean == self.mean[b]) & (idx < b)))).sum()) if seen[b] else 1
            v = 1.0
            for _ in range(self.power):
                v = v * (1.0 / float(rank))
            w.append(v)
        W = 0.0
        for v in w:
            W = W + v
        mix = float(self.mix)
        acc = 0.0
        for b in range(B):
            acc = acc + ((1.0 - mix) * w[b] / W + mix / float(B))
            self.cdf[b] = int(np.floor(16777216.0 * acc))
        self.cdf[B - 1] = ONE


# ---- the cases the host and the GPU tests share
def grid_bins(B):
    """B bins over speed (and tilt for B = 256: 16 x 16), the other axes ranges."""
    from isaacgym_amd import curriculum
    if B == 256:
        return curriculum.grid({"serve_speed": (6.0, 9.0, 16), "serve_tilt": (-8.0, 8.0, 16)})
    return curriculum.grid({"serve_speed": (6.0, 9.0, B)})


def scripted(steps, num_envs, reset_rows, num_agents, seed=11, p=0.15):
    """(rew [steps, A*N] f32, reset [steps, reset_rows*N] int64).  Each env ends a game with probability p per step; the words are 1, 2 and
    1 << 32 (the low half alone would read as zero); with two rows per env, agent 1's rows carry stray words and rewards of their own that
    nothing may read.  Step 6: every env ends a game; step 7: none does.  A few rewards are inf / nan / beyond 2^31: games to be dropped."""
    rng = np.random.default_rng(seed)
    fire = rng.random((steps, num_envs)) < p
    if steps > 7:
        fire[6], fire[7] = True, False
    word = np.array([1, 2, 1 << 32], I64)[(np.arange(steps)[:, None] + np.arange(num_envs)[None, :]) % 3]
    reset = np.zeros((steps, reset_rows * num_envs), I64)
    reset[:, ::reset_rows] = np.where(fire, word, 0)
    if reset_rows == 2:
        reset[:, 1::2] = np.where(rng.random((steps, num_envs)) < 0.3, 7, 0)
    rew = np.zeros((steps, num_agents * num_envs), F32)
    rew[:, ::num_agents] = rng.normal(0.0, 3.0, (steps, num_envs)).astype(F32)
    if num_agents == 2:
        rew[:, 1::2] = 1e6
    for k, bad in enumerate((np.inf, np.nan, 3e9, -3e9)):
        if steps > 12 + k and num_envs > k:
            rew[12 + k, k * num_agents] = bad
    return rew, reset


def run(cur, rew, reset, horizon, update=True):
    """Drive a HostCurric / NumpyCurric over the scripted steps in horizons of `horizon` steps (fold + update after each).
    -> list per step of (words(), fin_bin row, fin_q row of the finished envs), list per horizon of tot."""
    steps, n = rew.shape[0], cur.num_envs
    per_step, per_horizon = [], []
    fin_bin, fin_q = np.full((horizon, n), -1, np.int32), np.zeros((horizon, n), I64)
    for t in range(steps):
        r = t % horizon
        cur.step(rew[t], reset[t], fin_bin[r], fin_q[r])
        per_step.append((cur.words(), fin_bin[r].copy(), np.where(fin_bin[r] >= 0, fin_q[r], 0)))
        if r == horizon - 1:
            tot = cur.fold(fin_bin, fin_q)
            per_horizon.append(tot.copy())
            if update:
                cur.update(tot)
    return per_step, per_horizon
