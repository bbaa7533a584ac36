"""ctypes binding of tests/csrc/libppenv_playactshim.so — the actuator-accounting arithmetic of the HIP kernels
(isaacgym_amd/csrc/ppenv_play_act_device.h) compiled for the host and summed in the kernels' order, built the way
play_pair_shim_binding.lib() builds the paired statistics' — and a numpy restatement of include/ppenv_play_act.h's rule, written from the
header's words alone.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import itertools
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd._lib import PLAY_ACT_FIELDS, PlayActGroup, PlayActInput, PlayActInputs, PlayActJoint, PlayActLimit, PlayActThresholds

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "play_act_shim.cpp")
_HDRS = [os.path.join(_HERE, "csrc", "butterfly_host.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_play_act_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_play_act.h"), os.path.join(_HERE, "..", "include", "ppenv_play_group.h"),
         os.path.join(_HERE, "..", "include", "ppenv_play.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_playactshim.so")
_lib = None
BLOCK = 256                                 # PPENV_PLAY_BLOCK


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.play_act_shim_sizeof_group.restype = L.play_act_shim_sizeof_joint.restype = L.play_act_shim_sizeof_inputs.restype = C.c_size_t
        L.play_act_shim_reset.restype = L.play_act_shim_accumulate.restype = None
        L.play_act_shim_reset.argtypes = [i32, i32, i32, vp, vp, vp]
        L.play_act_shim_accumulate.argtypes = [C.POINTER(PlayActInputs), vp, i32, i32, i32, i32, i64, vp, C.POINTER(PlayActThresholds), vp, vp, vp, vp]
        assert L.play_act_shim_sizeof_group() == C.sizeof(PlayActGroup) == 40 and L.play_act_shim_sizeof_joint() == C.sizeof(PlayActJoint) == 72
        assert L.play_act_shim_sizeof_inputs() == C.sizeof(PlayActInputs) == 96
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def limits_array(limits):
    """[D, 4] (lower, upper, effort, vel_limit) -> the float32 bytes of pp_play_act_limit[D]."""
    a = np.ascontiguousarray(limits, np.float32)
    assert a.ndim == 2 and a.shape[1] == 4 and C.sizeof(PlayActLimit) == 16
    return a


def np_input(view):
    """A float32 [N, D] numpy view with any strides -> PlayActInput (None -> the NULL action)."""
    if view is None:
        return PlayActInput(None, 0, 0)
    assert view.dtype == np.float32 and view.ndim == 2 and view.strides[0] % 4 == 0 and view.strides[1] % 4 == 0
    return PlayActInput(view.ctypes.data, view.strides[0] // 4, view.strides[1] // 4)


class HostAct:
    """isaacgym_amd.play.ActuatorStats in numpy, stepped by the kernel bodies on the CPU."""

    def __init__(self, envs_per_group, groups, num_agents, num_dofs, games_num, limits, thresholds):
        self.L = lib()
        self.S, self.G, self.A, self.D, self.games_num = int(envs_per_group), int(groups), int(num_agents), int(num_dofs), int(games_num)
        self.N = self.S * self.G
        self.limits = limits_array(limits)
        assert self.limits.shape[0] == self.D
        self.thr = PlayActThresholds(*[float(v) for v in thresholds])
        parts = (self.S + BLOCK - 1) // BLOCK
        self.state = np.full((1 + PLAY_ACT_FIELDS * self.D) * self.N, 0x55555555, np.uint32)      # garbage: reset() must clear it
        self.group = np.full(self.G * C.sizeof(PlayActGroup), 0x55, np.uint8)
        self.joint = np.full(self.G * self.D * C.sizeof(PlayActJoint), 0x55, np.uint8)
        self.partial = np.full(self.G * parts * (C.sizeof(PlayActGroup) + self.D * C.sizeof(PlayActJoint)), 0x55, np.uint8)
        self.reset()

    def reset(self):
        self.L.play_act_shim_reset(self.S, self.G, self.D, _p(self.state), _p(self.group), _p(self.joint))

    def accumulate(self, q, qd, tau, action, done):
        """q, qd, tau, action: float32 [N, D] views with any strides (action may be None); done: int64 [A * N]."""
        d = np.ascontiguousarray(done, np.int64)
        assert d.size == self.A * self.N and all(v is None or v.shape == (self.N, self.D) for v in (q, qd, tau, action))
        ins = PlayActInputs(np_input(q), np_input(qd), np_input(tau), np_input(action))
        self.L.play_act_shim_accumulate(C.byref(ins), _p(d), self.S, self.G, self.A, self.D, self.games_num, _p(self.limits), C.byref(self.thr),
                                        _p(self.state), _p(self.group), _p(self.joint), _p(self.partial))

    def state_bytes(self):
        """state, group totals, joint totals as bytes (ActuatorStats.state_bytes())."""
        return self.state.tobytes(), self.group.tobytes(), self.joint.tobytes()

    def read(self):
        return read_totals(self.group.tobytes(), self.joint.tobytes(), self.G, self.D)


def read_totals(group_bytes, joint_bytes, G, D):
    """-> (list of G PlayActGroup, list of G lists of D PlayActJoint)."""
    ng, nj = C.sizeof(PlayActGroup), C.sizeof(PlayActJoint)
    groups = [PlayActGroup.from_buffer_copy(group_bytes[g * ng:(g + 1) * ng]) for g in range(G)]
    joints = [[PlayActJoint.from_buffer_copy(joint_bytes[(g * D + d) * nj:(g * D + d + 1) * nj]) for d in range(D)] for g in range(G)]
    return groups, joints


# ---- the rule of include/ppenv_play_act.h in numpy
INT_FIELDS, SUM_FIELDS, MAX_FIELDS = ("c_effort", "c_vel", "c_limit", "c_clip"), ("abs_tau", "tau_sq", "power"), ("max_abs_tau", "max_abs_vel", "max_exc")


def numpy_act(q, qd, tau, action, dones, S, G, A, D, games_num, limits, thresholds):
    """q, qd, tau, action: float32 [steps, N, D] (action may be None); dones int64 [steps, A * N].  -> (per step a list of per-group games
    counts, final per-group dict(games, samples, launches, energy, energy_sq, terms; per joint field a [D] array), final running n [N])."""
    f32 = np.float32
    N = S * G
    lim = np.asarray(limits, f32)
    lower, upper, effort, vel_limit = lim[:, 0], lim[:, 1], lim[:, 2], lim[:, 3]
    effort_frac, vel_frac, margin, clip = (f32(v) for v in thresholds)
    effort_at, vel_at = (effort_frac * effort).astype(f32), (vel_frac * vel_limit).astype(f32)
    n = np.zeros(N, np.int32)
    run = {k: np.zeros((N, D), f32) for k in SUM_FIELDS + MAX_FIELDS}
    cnt = {k: np.zeros((N, D), np.int32) for k in INT_FIELDS}
    tot = [dict(games=0, samples=0, launches=0, energy=0.0, energy_sq=0.0, terms=0, **{k: np.zeros(D, np.int64) for k in INT_FIELDS},
                **{k: np.zeros(D, np.float64) for k in SUM_FIELDS}, max_abs_tau=np.zeros(D, f32), max_abs_vel=np.zeros(D, f32),
                max_exc=np.full(D, -np.inf, f32)) for _ in range(G)]
    games_after = []
    for s in range(dones.shape[0]):
        fin_all = dones[s].reshape(N, A)[:, 0] != 0
        for g in range(G):
            T = tot[g]
            if T["games"] >= games_num:
                continue                                                   # the freeze
            envs = np.arange(g * S, (g + 1) * S)
            smp, fin = envs[~fin_all[envs]], envs[fin_all[envs]]
            t, v, x = tau[s][smp], qd[s][smp], q[s][smp]
            at, av = np.abs(t), np.abs(v)
            run["abs_tau"][smp] += at
            run["tau_sq"][smp] += t * t
            run["power"][smp] += np.abs(t * v)
            run["max_abs_tau"][smp] = np.maximum(run["max_abs_tau"][smp], at)
            run["max_abs_vel"][smp] = np.maximum(run["max_abs_vel"][smp], av)
            exc = np.maximum(lower - x, x - upper)
            run["max_exc"][smp] = np.where((n[smp] == 0)[:, None], exc, np.maximum(run["max_exc"][smp], exc))
            cnt["c_effort"][smp] += at >= effort_at
            cnt["c_vel"][smp] += av >= vel_at
            cnt["c_limit"][smp] += exc >= -margin
            if action is not None:
                cnt["c_clip"][smp] += np.abs(action[s][smp]) >= clip
            n[smp] += 1
            for e in fin:                                                  # the folds
                T["games"] += 1
                T["samples"] += int(n[e])
                E = f32(0.0)
                for d in range(D):
                    E = f32(E + run["power"][e, d])
                T["energy"] += float(E)
                T["energy_sq"] += float(E) * float(E)
                T["terms"] += 1
                for k in SUM_FIELDS:
                    T[k] += run[k][e].astype(np.float64)
                for k in INT_FIELDS:
                    T[k] += cnt[k][e]
                T["max_abs_tau"] = np.maximum(T["max_abs_tau"], run["max_abs_tau"][e])
                T["max_abs_vel"] = np.maximum(T["max_abs_vel"], run["max_abs_vel"][e])
                if n[e] > 0:
                    T["max_exc"] = np.maximum(T["max_exc"], run["max_exc"][e])
                n[e] = 0
                for k in run:
                    run[k][e] = 0.0
                for k in cnt:
                    cnt[k][e] = 0
            T["launches"] += 1
        games_after.append([T["games"] for T in tot])
    return games_after, tot, n


def check_totals(groups, joints, want, what=""):
    """HostAct.read() (or ActuatorStats' bytes through read_totals) against numpy_act's totals: every integer equal, the fp32 maxima
    equal, every fp64 sum within n x 2^-52 x sum|term| of numpy's (check_sums' bound: the terms are the same fp64 numbers on both sides and
    non-negative, so sum|term| is the sum itself; n = the games folded)."""
    for g, (G_, J_, W) in enumerate(zip(groups, joints, want)):
        for k in ("games", "samples", "launches"):
            assert int(getattr(G_, k)) == W[k], (what, g, k, int(getattr(G_, k)), W[k])
        nt = max(W["terms"], 1)
        for k in ("energy", "energy_sq"):
            assert abs(getattr(G_, k) - W[k]) <= nt * 2.0 ** -52 * abs(W[k]), (what, g, k, getattr(G_, k), W[k])
        for d, j in enumerate(J_):
            for k in INT_FIELDS:
                assert int(getattr(j, k)) == int(W[k][d]), (what, g, d, k, int(getattr(j, k)), int(W[k][d]))
            for k in MAX_FIELDS:
                assert np.float32(getattr(j, k)) == W[k][d], (what, g, d, k, getattr(j, k), W[k][d])
            for k in SUM_FIELDS:
                assert abs(getattr(j, k) - W[k][d]) <= nt * 2.0 ** -52 * abs(W[k][d]), (what, g, d, k, getattr(j, k), W[k][d])
            assert j.reserved == 0.0


# ---- the cases the host and the GPU tests share
STEPS = 40
GROUPS = 3
WORDS = (1, 2, 1 << 32)
THRESHOLDS = (0.98, 0.98, 0.02, 1.0)        # effort_frac, vel_frac, limit_margin, action_clip
#         S         (D, A)                        layout          action
CASES = list(itertools.product((1, 65, 257), ((7, 1), (14, 2), (27, 1)), ("soa", "aos"), (True, False)))


def case_id(case):
    S, (D, A), layout, act = case
    return f"S{S}-D{D}-A{A}-{layout}-{'act' if act else 'noact'}"


def games_num_of(S):
    """Small enough that group 0 freezes mid-stream while group 1 (which hardly finishes anything) never does."""
    return 2 if S == 1 else 3 * S


def case_limits(D):
    d = np.arange(D, dtype=np.float32)
    return np.stack([-1.0 - 0.1 * d, 1.0 + 0.05 * d, 25.0 + d, 37.0 - 0.5 * d], axis=1).astype(np.float32)


def streams(S, A, D, steps=STEPS, G=GROUPS, seed=23):
    """-> q, qd, tau, action float32 [steps, N, D], dones int64 [steps, A * N].  The done words are play_shim_binding.scripted_dones' (1, 2 and
    2^32) with, where a group has envs enough, env 3 of every group never finishing and env 2 finishing every other step; group 0's first
    env also finishes in steps 3 AND 4 (a game of length 1), and group 1 keeps only its env 2 and one finish of its first env in step 30.
    Torques are clamped to the effort limit (values exactly on it), speeds and positions reach past their limits, actions past 1."""
    import play_shim_binding as ps
    N = S * G
    dones = ps.scripted_dones(steps, N, A, words=WORDS, seed=seed).reshape(steps, N, A)
    dones[:, S:2 * S, :] = 0
    dones[30, S, :] = 2
    dones[3:5, 0, :] = 1 << 32
    if S > 3:
        dones[:, 3::S, :] = 0
        dones[::2, 2::S, :] = 1 << 32
    rng = np.random.default_rng(seed + 1)
    lim = case_limits(D)
    tau = np.clip(rng.standard_normal((steps, N, D)) * 0.6 * lim[:, 2], -lim[:, 2], lim[:, 2]).astype(np.float32)
    qd = (rng.standard_normal((steps, N, D)) * 0.5 * lim[:, 3]).astype(np.float32)
    q = (lim[:, 0] - 0.05 + rng.random((steps, N, D)) * (lim[:, 1] - lim[:, 0] + 0.1)).astype(np.float32)
    action = (rng.standard_normal((steps, N, D)) * 0.8).astype(np.float32)
    return q, qd, tau, action, dones.reshape(steps, N * A)


def pack(layout, q, qd, tau, action):
    """One step's canonical [N, D] arrays in the env's own layout -> four [N, D] VIEWS of freshly packed buffers (and the buffers, to keep
    them alive): "soa" is the 7-dof tasks' [D][N] planes; "aos" the 27-dof task's dof_states [N, D, 2] and dof_force [N, D].  The action
    tensor is row-major [N, D] in both (with two agents: rows 2e + a of D / 2)."""
    N, D = q.shape
    act = None if action is None else np.ascontiguousarray(action)
    if layout == "soa":
        bufs = [np.ascontiguousarray(a.T) for a in (q, qd, tau)]
        views = [b.T for b in bufs]
    else:
        states = np.ascontiguousarray(np.stack([q, qd], axis=2))
        bufs = [states, np.ascontiguousarray(tau)]
        views = [states[:, :, 0], states[:, :, 1], bufs[1]]
    return views + [act], bufs + [act]
