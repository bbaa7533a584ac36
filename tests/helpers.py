"""Shared helpers for the parity tests."""
import ctypes
import os
import subprocess

import numpy as np

from isaacgym_amd import scene

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BODY_IDS = [0, 31, 32, 33, 34, 35, 36, 37, 38, 39]

# fp32 tolerances of the parity bar (BASELINE.json north_star: "fp32, rtol 1e-4")
RTOL = 1e-4
ATOL = 1e-5


def build_shim(src, out, deps, flags):
    """A host shim (tests/csrc/*.cpp: kernel arithmetic compiled for the CPU) as a CDLL: g++ of `src` -> `out` with `flags` (the shim's
    own floating-point switches; the parity tolerances were set against them) when `out` is missing or older than `src` / `deps`.
    Built aside and renamed: another test process never loads half a file."""
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [src] + list(deps)):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17"] + list(flags) + ["-Wno-unknown-pragmas", "-o", tmp, src],
                       check=True, capture_output=True)
        os.replace(tmp, out)
    return ctypes.CDLL(out)


def load_golden(variant):
    return np.load(os.path.join(GOLDEN_DIR, f"post_physics_{variant}.npz"))


def golden_config(variant, g, **kw):
    """The task config the golden fixture was generated with (tools/gen_golden.py)."""
    cfg = scene.default_task_cfg(variant)
    cfg["env"]["episodeLength"] = int(g["episode_length"])
    n = g["out_rew"].shape[1]
    return scene.build_config(variant, cfg=cfg, num_envs=n, **kw)


def expand_bodies(compact):
    """[N,10,13] observed rows -> the reference's [N,42,13] rigid-body tensor (other rows zero)."""
    n = compact.shape[0]
    full = np.zeros((n, scene.NUM_BODIES, 13), np.float32)
    full[:, BODY_IDS, :] = compact
    return full


PARITY_REPORT = []      # one line per probe-using test: printed in the terminal summary by tests/conftest.py
_WORST = [0.0]          # largest |err| / tolerance any assert_close has retained since the last ExclusionLog was opened


class ExclusionLog:
    """Book-keeping of a test that uses SensitivityProbe: how many env-steps the probe excluded, how close to the tolerance the
    worst RETAINED comparison came, and how check_excluded judged the excluded ones (matched the main oracle run, matched a jittered
    run, unmatched); asserts the exclusion bound (None: no bound) and that every excluded env-step was checked and matched, and
    leaves one line for the terminal summary."""

    def __init__(self, name, bound):
        self.name, self.bound, self.excluded, self.total = name, bound, 0, 0
        self.matched_main, self.matched_jittered, self.in_envelope, self.unmatched = 0, 0, 0, 0
        _WORST[0] = 0.0

    def add(self, keep):
        self.excluded += int((~keep).sum())
        self.total += int(keep.size)

    def close(self):
        frac = self.excluded / max(self.total, 1)
        checked = self.matched_main + self.matched_jittered + self.in_envelope + self.unmatched
        bound = "no bound" if self.bound is None else f"bound {100 * self.bound:.2f} %"
        line = (f"{self.name}: probe excluded {self.excluded} of {self.total} env-steps ({100 * frac:.3f} %, {bound}); "
                f"worst retained error = {_WORST[0]:.3f} x tolerance; excluded env-steps matched main oracle {self.matched_main}, "
                f"matched a jittered run {self.matched_jittered}, " + (f"within the runs' envelope {self.in_envelope}, " if self.in_envelope else "") +
                f"unmatched {self.unmatched}")
        PARITY_REPORT.append(line)
        print(line)
        assert self.bound is None or frac <= self.bound, line
        assert checked == self.excluded, f"{line}: {self.excluded - checked} excluded env-steps never reached check_excluded"
        assert self.unmatched == 0, line


def assert_close(actual, expected, what, rtol=RTOL, atol=ATOL):
    actual = np.asarray(actual, dtype=np.float64)
    expected = np.asarray(expected, dtype=np.float64)
    err = np.abs(actual - expected)
    tol = atol + rtol * np.abs(expected)
    if err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
        _WORST[0] = max(_WORST[0], float(np.max(ratio)))
    bad = err > tol
    if bad.any():
        idx = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} beyond rtol={rtol} atol={atol}; worst at {idx}: "
                             f"got {actual[idx]!r} want {expected[idx]!r}")


# Characteristic magnitude of each state tensor.  The fp32 parity bar is rtol 1e-4; for values that
# are the small difference of large ones (a joint velocity swinging from the 37 rad/s limit to ~0 in
# one step, a ball leaving a paddle that moves at 15 m/s) the absolute error is bounded by
# 1e-4 x the tensor's range, which is what `atol = RTOL * scale` expresses.
SCALES = {
    "dof_pos": 3.1416,    # rad, joint limits
    "dof_vel": 37.0,      # rad/s, velocity limit
    "dof_force": 25.0,    # N m, effort limit
    "ball_pos": 3.0,      # m
    "ball_quat": 4.0,     # the step rotates the ball by |w| dt <= 500 rad/s / 60 Hz = 8 rad: q moves by half of that, and an rtol error in w shows in q at that scale
    "ball_vel": 10.0,     # m/s
    "ball_spin": 500.0,   # rad/s: surface speed / radius = 10 m/s / 0.02 m, i.e. the same bound as ball_vel
}
BALL_ROWS = {"ball_pos": slice(0, 3), "ball_quat": slice(3, 7), "ball_vel": slice(7, 10), "ball_spin": slice(10, 13)}


# Round 2: the absolute part of the 7-dof tolerances is a QUARTER of "1e-4 x the tensor's range".  The probe-using tests print the
# worst error they retain (ExclusionLog); on the GPU it is < 0.1 x the round-1 tolerance, i.e. < 0.4 x this one.
ATOL_FRACTION = 0.25
for _k in list(SCALES):
    SCALES[_k] *= ATOL_FRACTION


def assert_state_close(got, want, what):
    """got / want: objects with SoA arrays dof_pos, dof_vel, dof_force [7,N], ball [13,N]."""
    for name in ("dof_pos", "dof_vel", "dof_force"):
        assert_close(getattr(got, name), getattr(want, name), f"{what}: {name}", atol=RTOL * SCALES[name])
    for name, rows in BALL_ROWS.items():
        a, b = got.ball[rows], want.ball[rows]
        if name == "ball_quat":   # q and -q are the same rotation
            sign = np.sign(np.sum(a * b, axis=0, keepdims=True))
            a = a * np.where(sign == 0, 1, sign)
        assert_close(a, b, f"{what}: {name}", atol=RTOL * SCALES[name])


def obs_atol():
    """Per-column atol of an obs row: body pos (30), body vel (30), dof_pos (7), 0.1*dof_vel (7), ball pos (3), ball vel (3)."""
    a = np.empty(scene.NUM_OBS, np.float64)
    a[0:30] = RTOL * 1.0 * ATOL_FRACTION        # arm reach ~1 m
    a[30:60] = RTOL * 20.0 * ATOL_FRACTION      # link velocities up to ~20 m/s when the arm flails at the velocity limits
    a[60:67] = RTOL * SCALES["dof_pos"]
    a[67:74] = RTOL * SCALES["dof_vel"] * 0.1
    a[74:77] = RTOL * SCALES["ball_pos"]
    a[77:80] = RTOL * SCALES["ball_vel"]
    return a


def reward_atol(config):
    """Reward scale: alpha * |vx| dominates (TT:1159); the power term is c * sum|tau qd| <= c * 7 * 25 * 37."""
    return RTOL * max(ATOL_FRACTION, abs(config.alpha_velocity_reward) * SCALES["ball_vel"], abs(config.power_coefficient) * 6475.0 * ATOL_FRACTION)


class SensitivityProbe:
    """Finds the envs whose step sits on a discontinuity of the physics specification.

    The specification has hard switches (contact activation `s < contact_offset`, the bounce threshold, the limit
    clamps): when an env lands within fp32 rounding of one, the fp64 oracle and the fp32 kernel may take different
    branches and legitimately differ by far more than rtol 1e-4 (reproduced identically by all kernel schedules).  The probe steps a second oracle from the same state with the
    continuous inputs jittered by a few 1e-6 relative; an env whose *oracle* result moves by more than the parity tolerance
    under that jitter is excluded from the comparison with the main oracle run of that step, and checked instead by
    check_excluded: its kernel step must match, integers and continuous outputs, the main run or one of a few jittered runs."""

    def __init__(self, oracle_lib, config, rel=1e-6, seed=99):   # ~10 ulp of fp32: the size of the kernel's own rounding after ~1e3 operations
        self.o2 = oracle_lib.OracleEnv(config, threads=8)
        self.rew_atol = reward_atol(config)
        self.rel, self.seed = rel, seed
        self.rng = np.random.default_rng(seed)

    def sensitive(self, state_blob, actions, o_after):
        """state_blob: oracle state before the step; o_after: the main oracle after its step.  -> bool [N]"""
        o2 = self.o2
        n = o2.num_envs
        bad = np.zeros(n, bool)
        for _ in range(2):
            o2.set_state(state_blob)
            for arr in (o2.dof_pos, o2.dof_vel, o2.ball):
                arr *= (1.0 + self.rel * self.rng.uniform(-1, 1, arr.shape)).astype(np.float32)
            o2.step(actions)
            for name in ("dof_pos", "dof_vel", "dof_force"):
                a, b = getattr(o2, name), getattr(o_after, name)
                bad |= (np.abs(a - b) > 0.3 * (RTOL * SCALES[name] + RTOL * np.abs(b))).any(axis=0)
            for name, rows in BALL_ROWS.items():
                if name == "ball_quat":
                    continue
                a, b = o2.ball[rows], o_after.ball[rows]
                bad |= (np.abs(a - b) > 0.3 * (RTOL * SCALES[name] + RTOL * np.abs(b))).any(axis=0)
            A = o2.num_agents
            # the reward reads the pre-reset ball velocity, which the state of an env that reset this step no longer shows
            drew = np.abs(o2.rew_buf - o_after.rew_buf) > 0.3 * (self.rew_atol + RTOL * np.abs(o_after.rew_buf))
            bad |= drew.reshape(n, A).any(axis=1)
            bad |= (o2.reset_buf.reshape(n, A) != o_after.reset_buf.reshape(n, A)).any(axis=1)
            bad |= (o2.flags.reshape(A, n) != o_after.flags.reshape(A, n)).any(axis=0)
        return bad

    def check_excluded(self, log, t, state_blob, actions, o_after, got, keep, oa, ra, k=8):
        """check_excluded for the envs this probe set aside (~keep): `got` is the kernel's state view after the step, `o_after` the
        main oracle's, `state_blob` the oracle state before it; oa / ra the test's own obs / reward tolerances.  The jittered runs are
        steps of the probe's second oracle (which carries any randomisation tables / gravity the test gave it)."""
        envs = np.flatnonzero(~keep)
        if envs.size == 0:
            return
        A = o_after.num_agents
        rng = np.random.default_rng([self.seed, t])
        o2 = self.o2

        def sample(scale):
            o2.set_state(state_blob)
            for arr in (o2.dof_pos, o2.dof_vel, o2.ball):
                arr *= (1.0 + scale * rng.uniform(-1, 1, arr.shape)).astype(np.float32)
            o2.step(actions)
            return step_outputs(o2, envs, A)
        check_excluded(log, f"{log.name}, step {t}", envs, step_outputs(got, envs, A), step_outputs(o_after, envs, A), sample,
                       step_spec(oa, ra), STEP_INTS, k=k)


# ---------------------------------------------------------------------------------------------------------------------------------
# The env-steps a probe sets aside are checked too: the kernel's step must be one the ORACLE takes from the same state, either its
# main run or one of K runs with the continuous inputs jittered (scales cycling through JITTER_SCALES), with the same integers and
# every continuous output within the test's own tolerances.  The cycle starts at 1e-7, about one fp32 ulp: on the steep part of a
# contact ramp (T3, host shim, step 32 of test_single_step_parity_vs_oracle: the pre-reset ball velocity in the reward) a 1e-6
# jitter already moves the oracle's reward by 10 x its tolerance, so only runs that move the inputs by the kernel's own rounding
# can land near the kernel's result.  Outputs are dicts of arrays with the env first, restricted to the
# excluded envs; a spec is a list of (key, atol, quat): the tolerance is atol + RTOL |want| as in assert_close (atol may instead be
# a callable of the wanted outputs returning the whole tolerance), quat = the last axis holds quaternions, compared up to sign.
JITTER_SCALES = (1e-7, 3e-7, 1e-6, 3e-6, 1e-5)
STEP_INTS = ("reset", "progress", "flags", "episode")


def step_outputs(view, envs, num_agents=1):
    """The 7-dof / 4-actor step's outputs of `envs` from a state view (oracle / DevView / ShimEnv); per agent where there are two."""
    n, A = view.ball.shape[1], num_agents
    d = {name: getattr(view, name)[:, envs].T for name in ("dof_pos", "dof_vel", "dof_force")}
    for name, rows in BALL_ROWS.items():
        d[name] = view.ball[rows][:, envs].T
    d["obs"] = view.obs_buf.reshape(n, A, -1)[envs]
    d["rew"] = view.rew_buf.reshape(n, A)[envs]
    d["reset"] = view.reset_buf.reshape(n, A)[envs]
    d["progress"] = view.progress_buf.reshape(n, A)[envs]
    d["flags"] = view.flags.reshape(-1, n)[:, envs].T
    d["episode"] = view.episode[envs]
    return {k: np.array(v) for k, v in d.items()}


def step_spec(oa, ra):
    """assert_state_close + the obs / reward comparisons of the 7-dof parity tests."""
    return ([(name, RTOL * SCALES[name], False) for name in ("dof_pos", "dof_vel", "dof_force")] +
            [(name, RTOL * SCALES[name], name == "ball_quat") for name in BALL_ROWS] + [("obs", oa, False), ("rew", ra, False)])


def close_rows(got, want, tol, quat=False):
    """Per-env form of assert_close: got / want [M, ...], tol broadcastable to them.  -> (ok [M], worst |err| / tol [M]); a
    non-finite output is never ok and its ratio is inf."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if quat:
        sign = np.sign(np.sum(g * w, axis=-1, keepdims=True))
        g = g * np.where(sign == 0, 1, sign)
    err = np.abs(g - w)
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(g), ratio, np.inf).reshape(len(g), -1)
    ok = ((err <= tol) & np.isfinite(g)).reshape(len(g), -1).all(axis=1)
    return ok, ratio.max(axis=1, initial=0.0)


def _judge(got, want, spec, ints):
    m = len(next(iter(got.values())))
    ints_ok = np.ones(m, bool)
    for key in ints:
        ints_ok &= (np.asarray(got[key]) == np.asarray(want[key])).reshape(m, -1).all(axis=1)
    ok, ratios = ints_ok.copy(), np.zeros((m, len(spec)))
    for j, (key, atol, quat) in enumerate(spec):
        tol = atol(want) if callable(atol) else atol + RTOL * np.abs(np.asarray(want[key], np.float64))
        o, ratios[:, j] = close_rows(got[key], want[key], tol, quat)
        ok &= o
    return ints_ok, ok, ratios


def _within_envelope(got, samples, spec, ints):
    """-> ok [M]: every continuous output lies between the smallest (value - tolerance) and the largest (value + tolerance) of the
    samples whose integers equal the kernel's (there must be one), and is finite."""
    m = len(next(iter(got.values())))
    same = [np.all([(np.asarray(got[kk]) == np.asarray(s[kk])).reshape(m, -1).all(axis=1) for kk in ints], axis=0) if ints else np.ones(m, bool)
            for s in samples]
    ok = np.any(same, axis=0)
    for key, atol, quat in spec:
        g = np.asarray(got[key], np.float64)
        lo, hi = np.full(g.shape, np.inf), np.full(g.shape, -np.inf)
        for s, sm in zip(samples, same):
            w = np.asarray(s[key], np.float64)
            if quat:
                sign = np.sign(np.sum(g * w, axis=-1, keepdims=True))
                w = w * np.where(sign == 0, 1, sign)
            tol = np.broadcast_to(atol(s) if callable(atol) else atol + RTOL * np.abs(np.asarray(s[key], np.float64)), w.shape)
            use = sm.reshape((m,) + (1,) * (w.ndim - 1))
            lo, hi = np.where(use, np.minimum(lo, w - tol), lo), np.where(use, np.maximum(hi, w + tol), hi)
        ok &= ((g >= lo) & (g <= hi) & np.isfinite(g)).reshape(m, -1).all(axis=1)
    return ok


def check_excluded(log, what, envs, got, main, sample, spec, ints, k=8, envelope=False):
    """Checks the env-steps a probe set aside: each must (a) have finite outputs and match, in one sample, (b) every integer output
    (`ints`) exactly and (c) every continuous output of `spec` at the test's tolerances.  The samples are the main oracle run
    (`main`) first, then sample(scale) for scale cycling through JITTER_SCALES, up to k jittered runs — drawn only while some env
    is still unmatched.  envelope=True (only for set-aside steps whose oracle result is spread over several values even at a 1e-7
    jitter, see run_chain_step_parity): an env that no single sample matches may instead lie within the envelope of the k + 1 runs
    that have its integers (_within_envelope); ExclusionLog counts those separately.  Counts the outcome into `log` (ExclusionLog)
    and raises AssertionError naming the first unmatched env, its integers and the nearest sample.  got / main / sample(): output
    dicts of the envs `envs` (see above)."""
    envs = np.asarray(envs)
    if envs.size == 0:
        return
    ints_ok, ok, ratios = _judge(got, main, spec, ints)
    main_ok = ok.copy()
    pending = ~ok
    # the nearest sample of every env: integers equal first, then the smallest worst ratio
    near = [(not i, float(r.max(initial=0.0)), 0, main, r) for i, r in zip(ints_ok, ratios)]
    drawn = [main]
    j = 0
    while pending.any() and j < k:
        want = sample(JITTER_SCALES[j % len(JITTER_SCALES)])
        drawn.append(want)
        j += 1
        ints_ok, ok, ratios = _judge(got, want, spec, ints)
        for e in np.flatnonzero(pending):
            cand = (not ints_ok[e], float(ratios[e].max(initial=0.0)), j, want, ratios[e])
            if cand[:2] < near[e][:2]:
                near[e] = cand
        pending &= ~ok
    in_envelope = pending & _within_envelope(got, drawn, spec, ints) if envelope and pending.any() else np.zeros_like(pending)
    log.matched_main += int(main_ok.sum())
    log.matched_jittered += int((~main_ok & ~pending).sum())
    log.in_envelope = getattr(log, "in_envelope", 0) + int(in_envelope.sum())
    pending &= ~in_envelope
    log.unmatched += int(pending.sum())
    if pending.any():
        e = int(np.flatnonzero(pending)[0])
        _, _, js, want, r = near[e]
        worst = int(np.argmax(r))
        key = spec[worst][0]
        g, w = np.asarray(got[key][e], np.float64).ravel(), np.asarray(want[key][e], np.float64).ravel()
        diff = np.where(np.isfinite(g), np.abs(g - w), np.inf)
        at = int(np.argmax(diff)) if diff.size else 0
        nonfinite = [kk for kk in got if not np.all(np.isfinite(np.asarray(got[kk], np.float64)[e]))]
        raise AssertionError(
            f"{what}: excluded env {int(envs[e])} matches neither the main oracle run nor any of {j} jittered runs "
            f"({int(pending.sum())} of {envs.size} excluded envs unmatched); non-finite outputs: {nonfinite or 'none'}; "
            f"kernel integers {({kk: np.asarray(got[kk][e]).tolist() for kk in ints})}; nearest sample "
            f"{'main oracle run' if js == 0 else f'jittered run {js}'} with integers {({kk: np.asarray(want[kk][e]).tolist() for kk in ints})}, "
            f"worst {key} at {r[worst]:.3g} x tolerance, element {at}: kernel {g[at]!r} oracle {w[at]!r}")


class _Masked:
    pass


def mask_envs(view, keep, num_agents=1):
    """A copy of a state view (oracle / DevView / ShimEnv attributes) restricted to the envs in `keep` (bool [N])."""
    m = _Masked()
    rows = np.repeat(keep, num_agents)
    for name in ("dof_pos", "dof_vel", "dof_force", "ball"):
        setattr(m, name, getattr(view, name)[:, keep])
    m.flags = view.flags[..., keep]
    m.episode = view.episode[keep]
    for name in ("progress_buf", "reset_buf", "rew_buf", "obs_buf"):
        setattr(m, name, getattr(view, name)[rows])
    return m
