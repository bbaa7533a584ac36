"""ctypes binding of tests/csrc/libppenv_adrshim.so — the ADR arithmetic of the HIP kernels (isaacgym_amd/csrc/ppenv_dr_adr_device.h)
compiled for the host, built the way serve_curric_shim_binding.lib() builds the serve curriculum's — and `NumpyAdr`, the rule of
include/ppenv_dr_adr.h restated in numpy from the header's words.  The fold is the serve curriculum's on both sides (the header says so).
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

import serve_curric_shim_binding as scb
from helpers import build_shim
from isaacgym_amd import _lib, scene
from serve_curric_shim_binding import np_q, same_words, scripted  # noqa: F401  (the cases the tests share)

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "adr_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", n) for n in ("ppenv_dr_adr_device.h", "ppenv_dr_device.h", "ppenv_serve_curric_device.h",
                                                                       "ppenv_serve_device.h", "ppenv_device.h")] + \
        [os.path.join(_HERE, "..", "include", n) for n in ("ppenv_dr_adr.h", "ppenv_dr.h", "ppenv_serve_curric.h", "ppenv_serve.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_adrshim.so")
_shim = None

U32, U64, F32, F64, I32, I64 = np.uint32, np.uint64, np.float32, np.float64, np.int32, np.int64
ONE = 1 << 24
DROPPED = scb.DROPPED
FLT_MAX = float(np.finfo(F32).max)
STATE = ("range", "draws", "slot", "ret", "acc_n", "acc_q", "games", "dropped", "mean", "widened", "narrowed")


def lib():
    global _shim
    if _shim is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        i32, u32, u64, vp, f32, f64 = C.c_int32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_float, C.c_double
        ap, sp = C.POINTER(_lib.Adr), C.POINTER(_lib.AdrState)
        for name in ("layout", "consts", "fill", "step", "update"):
            getattr(L, f"adr_shim_{name}").restype = None
        L.adr_shim_layout.argtypes = L.adr_shim_consts.argtypes = [vp]
        L.adr_shim_invalid.argtypes = [ap, f64, C.POINTER(i32)]
        L.adr_shim_thr.restype, L.adr_shim_thr.argtypes = u32, [f64]
        L.adr_shim_u24.restype, L.adr_shim_u24.argtypes = u32, [u64, u32, u32, u32]
        L.adr_shim_uniform.restype, L.adr_shim_uniform.argtypes = f32, [u64, u32, u32, u32]
        L.adr_shim_slot.restype, L.adr_shim_slot.argtypes = i32, [u64, u32, u32, u32, i32]
        L.adr_shim_fill.argtypes = [ap, i32, sp]
        L.adr_shim_step.argtypes = [ap, vp, vp, sp, vp, vp]
        L.adr_shim_update.argtypes = [ap, i32, vp, sp]
        _shim = L
    return _shim


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def dim(rows, start, limit, step):
    return dict(rows=int(rows), start=(float(start[0]), float(start[1])), limit=(float(limit[0]), float(limit[1])), step=float(step))


def host_adr(num_envs, dims, table_ptrs, reset_rows=1, num_agents=1, seed=0, env_id_offset=0, boundary_frac=0.25, min_games=1, t_low=-1.0, t_high=1.0,
             n_dims=None):
    """pp_dr_adr as adr.AutoRandomizer builds it, thr filled in as the upload computes it; n_dims: an override, for the refusals."""
    A = _lib.Adr(num_envs=num_envs, env_id_offset=env_id_offset, seed=seed & 0xFFFFFFFFFFFFFFFF, reset_rows=reset_rows, num_agents=num_agents,
                 dims=len(dims) if n_dims is None else n_dims, thr=0, min_games=min_games, t_low=t_low, t_high=t_high)
    for m, d, ptr in zip(A.dim, dims, table_ptrs):
        m.table, m.rows = ptr, d["rows"]
        (m.start_lo, m.start_hi), (m.limit_lo, m.limit_hi), m.step = d["start"], d["limit"], d["step"]
    if 0.0 <= boundary_frac <= 1.0:
        A.thr = int(np.floor(np.float64(boundary_frac) * 16777216.0))
    return A


class _State:
    """The state arrays and the tables both restatements keep, and their comparison."""

    def _alloc(self, n, dims):
        D = len(dims)
        S = 2 * D + 1
        self.range = np.zeros((D, 2), F32)
        self.draws, self.slot, self.ret = np.zeros(n, I32), np.zeros(n, I32), np.zeros(n, F32)
        self.acc_n, self.acc_q, self.games, self.dropped = (np.zeros(S, I64) for _ in range(4))
        self.mean, self.widened, self.narrowed = np.zeros(S, F32), np.zeros(S, I32), np.zeros(S, I32)
        self.tables = [np.ones((d["rows"], n), F32) for d in dims]

    def words(self):
        """{name: the array's words as integers} of every state array and every table."""
        out = {k: np.ascontiguousarray(getattr(self, k)).view(U32 if getattr(self, k).dtype.itemsize == 4 else U64).copy() for k in STATE}
        out.update({f"table{d}": t.view(U32).copy() for d, t in enumerate(self.tables)})
        return out


class HostAdr(_State):
    """adr.AutoRandomizer in numpy, stepped by the kernel bodies on the CPU."""

    def __init__(self, num_envs, dims, **kw):
        self.L = lib()
        n = self.num_envs = int(num_envs)
        self.dims, self.D, self.slots = dims, len(dims), 2 * len(dims) + 1
        self._alloc(n, dims)
        self.adr = host_adr(n, dims, [t.ctypes.data for t in self.tables], **kw)
        which = C.c_int32(0)
        assert self.L.adr_shim_invalid(C.byref(self.adr), kw.get("boundary_frac", 0.25), C.byref(which)) == 0
        self.reset_rows, self.num_agents = self.adr.reset_rows, self.adr.num_agents
        self.state = _lib.AdrState(*(getattr(self, k).ctypes.data for k in STATE))
        self.fill()

    def fill(self):
        self.L.adr_shim_fill(C.byref(self.adr), self.D, C.byref(self.state))

    def step(self, rew, reset, fin_slot_t, fin_q_t):
        """fin_slot_t [N] int32 / fin_q_t [N] int64: the caller's rows, written in place."""
        rew, reset = np.ascontiguousarray(rew, F32), np.ascontiguousarray(reset, I64)
        assert rew.size == self.num_agents * self.num_envs and reset.size == self.reset_rows * self.num_envs
        assert fin_slot_t.dtype == I32 and fin_q_t.dtype == I64 and fin_slot_t.flags.c_contiguous and fin_q_t.flags.c_contiguous
        self.L.adr_shim_step(C.byref(self.adr), _p(rew), _p(reset), C.byref(self.state), _p(fin_slot_t), _p(fin_q_t))

    def fold(self, fin_slot, fin_q):
        fin_slot, fin_q = np.ascontiguousarray(fin_slot, I32), np.ascontiguousarray(fin_q, I64)
        tot = np.zeros((3, self.slots), I64)
        scb.lib().curric_shim_fold(_p(fin_slot), _p(fin_q), fin_slot.size, self.slots, _p(tot))
        return tot

    def update(self, tot):
        tot = np.ascontiguousarray(tot, I64)
        assert tot.shape == (3, self.slots)
        self.L.adr_shim_update(C.byref(self.adr), self.D, _p(tot), C.byref(self.state))


def ubits(kseed, gid, episode, k):
    """rng_uniform's 24-bit integer in numpy (test_serve_plan_host.ubits)."""
    from test_serve_plan_host import ubits as u
    return u(kseed, gid, episode, k)


def np_slots(seed, gids, j, thr, D):
    """The slot of redraw j of the global env ids, from the header's words: the coin at index 512, the pick at 513."""
    sd = (int(seed) & 0xFFFFFFFFFFFFFFFF) ^ scene.DR_SEED_SALT
    gids, j = np.asarray(gids).astype(U32), np.asarray(j).astype(U32)
    worker = ubits(sd, gids, j, 512).astype(I64) < int(thr)
    b = (ubits(sd, gids, j, 513).astype(U64) * U64(2 * D)) >> U64(24)
    return np.where(worker, b.astype(I64), 2 * D).astype(I32)


def np_columns(seed, gids, j, d, rows, lo, hi):
    """[rows, len(gids)]: the interior values of table d — base * (hi - lo) + lo, each operation rounded to fp32, a zero stored as +0."""
    sd = (int(seed) & 0xFFFFFFFFFFFFFFFF) ^ scene.DR_SEED_SALT
    gids, j = np.asarray(gids).astype(U32), np.asarray(j).astype(U32)
    lo, hi = F32(lo), F32(hi)
    out = np.zeros((rows, gids.size), F32)
    for r in range(rows):
        base = ubits(sd, gids, j, d * 64 + r).astype(F32) * F32(1.0 / 16777216.0)
        v = (base * F32(hi - lo)).astype(F32) + lo
        out[r] = np.where(v == 0, F32(0), v)
    return out


class NumpyAdr(_State):
    """The rule in numpy, from the words of include/ppenv_dr_adr.h."""

    def __init__(self, num_envs, dims, reset_rows=1, num_agents=1, seed=0, env_id_offset=0, boundary_frac=0.25, min_games=1, t_low=-1.0, t_high=1.0):
        n = self.num_envs = int(num_envs)
        self.dims, self.D, self.slots = dims, len(dims), 2 * len(dims) + 1
        self.reset_rows, self.num_agents, self.seed, self.off = reset_rows, num_agents, seed & 0xFFFFFFFFFFFFFFFF, env_id_offset
        self.thr = int(np.floor(np.float64(boundary_frac) * 16777216.0))
        self.min_games, self.t_low, self.t_high = int(min_games), F32(t_low), F32(t_high)
        self._alloc(n, dims)
        self.fill()

    def draw(self, e, j, ranges):
        """Columns e of every table under `ranges` [D, 2]; -> the slots."""
        e = np.asarray(e)
        if e.size == 0:
            return np.zeros(0, I32)
        gids = self.off + e
        slots = np_slots(self.seed, gids, j, self.thr, self.D)
        for d, m in enumerate(self.dims):
            lo, hi = F32(ranges[d][0]), F32(ranges[d][1])
            cols = np_columns(self.seed, gids, j, d, m["rows"], lo, hi)
            for side, v in ((0, lo), (1, hi)):
                cols[:, slots == 2 * d + side] = v
            self.tables[d][:, e] = cols
        return slots

    def fill(self):
        self.range[:] = [[F32(m["start"][0]), F32(m["start"][1])] for m in self.dims]
        e = np.arange(self.num_envs)
        j = self.draws.copy()
        self.draws += 1
        self.draw(e, j, self.range)
        self.slot[:] = -1
        self.ret[:] = 0

    def step(self, rew, reset, fin_slot_t, fin_q_t):
        rew, reset = np.asarray(rew, F32).ravel(), np.asarray(reset, I64).ravel()
        self.ret = (self.ret + rew[::self.num_agents]).astype(F32)
        fired = reset[::self.reset_rows] != 0
        fin_slot_t[:] = np.where(fired, self.slot, -1)
        fin_q_t[fired] = np_q(self.ret[fired])
        self.ret[fired] = 0
        e = np.nonzero(fired)[0]
        j = self.draws[e].copy()
        self.draws[e] += 1
        self.slot[e] = self.draw(e, j, self.range)

    def fold(self, fin_slot, fin_q):
        fin_slot, fin_q = np.asarray(fin_slot).ravel(), np.asarray(fin_q, I64).ravel()
        tot = np.zeros((3, self.slots), I64)
        live = fin_slot >= 0
        drop = live & (fin_q == DROPPED)
        good = live & ~drop
        np.add.at(tot[0], fin_slot[good], 1)
        np.add.at(tot[1], fin_slot[good], fin_q[good])
        np.add.at(tot[2], fin_slot[drop], 1)
        return tot

    def update(self, tot):
        tot = np.asarray(tot, I64)
        for s in range(self.slots):
            n, q, dr = (int(tot[k][s]) for k in range(3))
            self.games[s] += n
            self.dropped[s] += dr
            self.acc_n[s] += n
            self.acc_q[s] += q
            if self.acc_n[s] < self.min_games:
                continue
            m = F32(F64(int(self.acc_q[s])) / (F64(65536.0) * F64(int(self.acc_n[s]))))
            self.mean[s] = m
            if s < 2 * self.D:
                d, side = s >> 1, s & 1
                dm = self.dims[d]
                step, v = F32(dm["step"]), self.range[d, side]
                if m >= self.t_high:
                    self.range[d, side] = min(F32(v + step), F32(dm["limit"][1])) if side else max(F32(v - step), F32(dm["limit"][0]))
                    self.widened[s] += 1
                elif m <= self.t_low:
                    self.range[d, side] = max(F32(v - step), F32(dm["start"][1])) if side else min(F32(v + step), F32(dm["start"][0]))
                    self.narrowed[s] += 1
            self.acc_n[s] = self.acc_q[s] = 0


# ---- the cases the host and the GPU tests share
DIMS_7 = [dim(7, (0.9, 1.1), (0.5, 1.5), 0.05), dim(7, (1.0, 1.0), (0.25, 2.0), 0.125), dim(7, (0.8, 1.25), (0.6, 1.4), 0.1),
          dim(1, (1.0, 1.0), (0.5, 1.0), 0.07), dim(1, (0.7, 1.3), (0.4, 1.6), 0.1)]
DIMS_27 = [dim(27, (0.9, 1.1), (0.5, 1.5), 0.05), dim(27, (1.0, 1.0), (0.25, 2.0), 0.125), dim(28, (0.8, 1.25), (0.6, 1.4), 0.1),
           dim(1, (1.0, 1.0), (0.5, 1.0), 0.07), dim(1, (0.7, 1.3), (0.4, 1.6), 0.1)]
DIMS_1 = [dim(7, (1.0, 1.0), (0.6, 1.4), 0.05)]
DIM_SETS = {"rows7": DIMS_7, "rows27": DIMS_27, "one": DIMS_1}
# the scripted rewards are N(0, 3) per step and a game lasts ~ 7 steps: returns spread over about +-8, so thresholds at +-1 see both moves
SCRIPT_KW = dict(boundary_frac=0.5, min_games=3, t_low=-1.0, t_high=1.0)


def run(adr, rew, reset, horizon, update=True, on_step=None):
    """Drive a HostAdr / NumpyAdr over the scripted steps in horizons of `horizon` steps (fold + update after each).
    -> list per step of (words(), fin_slot row, fin_q row of the finished envs), list per horizon of (tot, words() after the update)."""
    steps, n = rew.shape[0], adr.num_envs
    per_step, per_horizon = [], []
    fin_slot, fin_q = np.full((horizon, n), -1, I32), np.zeros((horizon, n), I64)
    for t in range(steps):
        r = t % horizon
        adr.step(rew[t], reset[t], fin_slot[r], fin_q[r])
        per_step.append((adr.words(), fin_slot[r].copy(), np.where(reset[t][::adr.reset_rows] != 0, fin_q[r], 0)))
        if r == horizon - 1:
            tot = adr.fold(fin_slot, fin_q)
            if update:
                adr.update(tot)
            per_horizon.append((tot.copy(), adr.words()))
    return per_step, per_horizon
