"""Scripted states that put the 7-dof (TT / TN / T3) and the 4-actor (T4) step on every hard switch of the drive (arm_substep, csrc/ppenv_device.h:
the explicit PD torque clamped at +-effort before the solve, dof_force clamped again at the end-of-substep velocity, the solved velocity clamped
at +-vel_limit, the position clamped at upper / lower with the velocity's outward part zeroed, and pd_target's clamp at clip_actions), and the
oracle-only book-keeping of the tests that use them (tests/test_joint_limits_host.py / _gpu.py).

The free-running rollouts reach the stops a handful of times on some joints and never on others, and the scripted suites stay away
from them on purpose.  Here every env has ONE focus joint, env % 7 (on T4 also the arm, (env // 7) % 2), and a drawn case that cycles with the
env's index (CYCLE: the share and the sign); its other joints are drawn as step_schedule_scenarios.start_state draws them and hold their pose
(start_state says where the oracle picks among several such draws).  Start poses stay inside [lower, upper]: the specification never leaves them.
The ball is parked at (10, 10, 5) and falls freely; nobody resets.  STEPS oracle steps, actions held.

Everything is decided from the ORACLE and the config, never from a kernel's output.  An env-step's cells (of its focus joint, per sign: "upper" is
towards the upper stop / +vel_limit / +effort / action > +clip) are read off the oracle's fp32 tensors before and after the step and off
COUNTERFACTUAL oracles stepped from the same state whose Config has (a) every effort x 100, (b) every vel_limit x 100, (c) lower / upper widened by
1 rad (with the actions rescaled so that the PD targets stay: widened_actions), (d) clip_actions x 100 — "reached" below means that the focus joint's dof_pos, dof_vel or dof_force of that counterfactual differs from
the stock oracle's by at least REACHED x the comparison tolerance (assert_state_close's):
  stop/substep0     not on the stop before, (c) reached, and a ONE-SUBSTEP oracle (substeps = 1, dt halved: the first substep as a step of its own)
                    from the same state ends with q == float32(limit).  (The end of the whole step need not show it: the second substep may
                    leave the stop again.)
  stop/later        not on the stop before, the one-substep oracle does not end on the stop, q == float32(limit) after the step, (c) reached: the
                    stop is taken in the second substep, from (q, qd) that the arm wave has handed over a boundary
  on_stop/held      on the stop and at rest before, the target on the stop (it cannot lie beyond; within 2 ulp, for mid-range + half-range is not
                    always the fp32 limit), q == limit and qd == 0 after, and (c) ends beyond the limit: something pushes into the stop
  on_stop/leaves    on the stop and at rest before, off it after, by at least REACHED x the tolerance of dof_pos or dof_vel
  speed_cap         (b) reached in dof_pos or dof_vel: the solved velocity exceeded vel_limit in some substep;  `cap_at_end`: moreover
                    qd == +-float32(vel_limit) after the step and (b)'s qd lies beyond it by REACHED x the tolerance
  torque/solve      the explicit torque kp (err - h qd) - kd qd of the step's start (fp64, from the tensors and the config, the env's own gains)
                    lies beyond +-effort, and (a) reached in dof_pos or dof_vel
  torque/reported   dof_force == +-float32(effort) after the step and (a)'s dof_force differs from it by REACHED x the tolerance (on a light joint the
                    unlimited twin moves so much faster that it reports LESS);  `torque_at_end`: (a)'s lies beyond it by that much
  action_clip       the focus action lies beyond +-clip_actions and (d) reached
`ends_on_stop` (q == limit and qd == 0 after the step), `cap_at_end` and `torque_at_end` mark where an end-of-step value is exact (exact_masks).
Whether a stop is DRAWN for substep 0 or later (the fraction 0.1 - 0.8 or 1.2 - 1.8) is kept in meta; the host test asserts that the drawn
reading and the one-substep oracle agree for every stop env.  The stop envs' targets stay on the stop: they feed on_stop/held in the steps that
follow."""
import functools
import types

import numpy as np

import ball_contact_scenarios as sc
from helpers import RTOL, SCALES, SensitivityProbe
from isaacgym_amd import scene
from ta_ball_contact_scenarios import REACHED

STEPS = 3
FLOOR = 8                    # kept env-steps every (joint, cell, sign) must reach
EXCLUDED_CAP = 0.02          # of a case's env-steps, as the other scripted suites
ENV_SEED = 13
VARIANTS = ("TT", "TN", "T3", "T4")
SIZES = (1, 63, 65, 130)     # step_schedule_scenarios.SIZES: compared, not counted
CELL_NAMES = ("stop/substep0", "stop/later", "on_stop/held", "on_stop/leaves", "speed_cap", "torque/solve", "torque/reported", "action_clip")
SIGNS = ("upper", "lower")
CELLS = tuple(f"{c}/{s}" for c in CELL_NAMES for s in SIGNS)
EXACT_CELLS = ("stop/substep0", "stop/later", "on_stop/held")      # q == limit and qd == 0 bit for bit; cap_at_end / torque/reported: qd / dof_force
# the shares of a sign: a stop is taken, and a stop left from rest, once per env, so these hold three shares each; on_stop/held is fed by the stop envs too
SHARES = ("stop/substep0",) * 3 + ("stop/later",) * 3 + ("on_stop/leaves",) * 3 + ("on_stop/held", "speed_cap", "torque/solve", "torque/solve", "torque/reported", "action_clip")
CYCLE = len(SHARES) * len(SIGNS)
CANDIDATES = 48              # drawn poses / targets of the other joints, of which the oracle picks the one that holds the focus joint on its stop longest
# The counted size: the smallest multiple of 7 x CYCLE = 210 that is no multiple of 64 at which the oracle holds the floor in every run below.  On T4
# the focus alternates between the arms, so a (joint, cell, sign) is counted over both arms and each arm must contribute.
COUNTED = 840
# scenario seed per (variant, n, dr) where 0 does not hold the floor: T3's shoulder roll exceeds its speed cap by REACHED x the tolerance in 7 env-steps
SEEDS = {("T3", 840, False): 1}


def seed_of(variant, n, dr):
    return SEEDS.get((variant, n, dr), 0)


def case_config(variant, n):
    return scene.build_config(variant, num_envs=n, seed=ENV_SEED)


def focus_of(cfg, n):
    """-> (joint [n], arm [n], dof row [n], sign [n] +1 / -1, share [n])."""
    env, A = np.arange(n), cfg.num_humanoids
    joint, arm = env % 7, (env // 7) % A
    case = (env // (7 * A)) % CYCLE
    return joint, arm, arm * 7 + joint, np.where(case % 2 == 0, 1.0, -1.0), case // 2


def joint_table(cfg):
    return {k: np.array([getattr(cfg.joint[j], k) for j in range(7)], np.float64) for k in ("lower", "upper", "kp", "kd", "effort", "vel_limit")}


def gain_tables(n, seed):
    """The randomised run: per-env kp / kd scales (the gains move the saturation point; the limits are not randomised), unit material and mass tables."""
    rng = np.random.default_rng([seed, 79])
    one = np.ones((7, n), np.float32)
    return dict(dof_stiffness_scale=rng.uniform(0.5, 1.5, (7, n)).astype(np.float32), dof_damping_scale=rng.uniform(0.5, 1.5, (7, n)).astype(np.float32),
                link_mass_scale=one, restitution_scale=np.ones(n, np.float32), friction_scale=np.ones(n, np.float32))


NO_NOISE = dict(action_noise_sigma=0.0, observation_noise_sigma=0.0)


def widened(cfg):
    c = sc._copy(cfg)
    for j in range(7):
        c.joint[j].lower -= 1.0
        c.joint[j].upper += 1.0
    return c


def widened_actions(cfg, actions):
    """The actions [n A, 7] whose targets under widened(cfg) are the stock config's targets of `actions` (the PD target is mid-range + half-range x the
    clipped action, and the widening keeps the mid-range), up to the fp32 rounding of the target."""
    J = joint_table(cfg)
    half = 0.5 * (J["upper"] - J["lower"])
    return (np.clip(actions.astype(np.float64), -float(cfg.clip_actions), float(cfg.clip_actions)) * (half / (half + 1.0))[None, :]).astype(np.float32)


def start_state(make, cfg, n, rng):
    """-> (o: an oracle in the drawn start state, actions [n A, 7] held over the run, meta).  make(config) builds an oracle (with the run's tables).

    Two things are settled by the oracle, because the draw alone cannot: (1) whether a joint on its stop with the target on the stop STAYS there is
    up to gravity and the other joints' reactions, so for the envs that are to stay (on_stop/held and the stops) CANDIDATES poses, rates and targets
    of the other joints are drawn and the one under which the focus joint, put on the stop at rest, is held for most of the STEPS steps is kept; the
    same for speed_cap, where a heavy joint gains less than REACHED x the tolerance of speed in a step unless the other joints help: the candidate
    under which the oracle without the cap ends its first step fastest is kept;
    (2) the drive's damping takes most of a light joint's velocity within one substep, so the distance to the stop is a fraction of what the joint
    TRAVELS — d1 in the first substep, d2 in the second, read off an oracle with the limits widened and its one-substep twin from the same state,
    three rounds of the fixed point — 0.1 - 0.8 of d1 for substep 0, d1 + (0.2 - 0.8) d2 for the later substep (a constant |v| makes these the
    fractions 0.1 - 0.8 and 1.2 - 1.8 of |v| h), with |v| = 3 - 20 rad/s at the start."""
    A, J = cfg.num_humanoids, joint_table(cfg)
    u = lambda lo_, hi_, shape=n: rng.uniform(lo_, hi_, shape)
    lo, hi = np.tile(J["lower"], A), np.tile(J["upper"], A)
    to_act = lambda q_: np.clip((q_ - 0.5 * (hi + lo)[:, None]) / (0.5 * (hi - lo))[:, None], -1, 1)
    q = np.clip(u(-0.6, 0.6, (7 * A, n)), (lo + 0.01)[:, None], (hi - 0.01)[:, None])
    qd = u(-2.0, 2.0, (7 * A, n))
    act = to_act(q)
    joint, arm, row, s, share = focus_of(cfg, n)
    env = np.arange(n)
    L, mid, half = np.where(s > 0, J["upper"][joint], J["lower"][joint]), 0.5 * (J["upper"] + J["lower"])[joint], 0.5 * (J["upper"] - J["lower"])[joint]
    L32 = np.where(s > 0, [cfg.joint[j].upper for j in joint], [cfg.joint[j].lower for j in joint]).astype(np.float32)   # what the kernels and the oracle read
    kind = np.array(SHARES)[share]
    stop, on_stop = np.isin(kind, ("stop/substep0", "stop/later")), np.isin(kind, ("on_stop/held", "on_stop/leaves"))
    back = mid - s * u(0.2, 0.6) * half                       # the far half of the range: the target on this stop saturates the drive
    fq = np.select([stop | on_stop, kind == "speed_cap", kind == "torque/reported", kind == "torque/solve"],
                   [L, back, mid - s * u(0.6, 0.9) * half, mid - s * u(0.3, 0.9) * half], L - s * u(0.05, 0.3))
    vlim = J["vel_limit"][joint]
    fqd = np.select([stop | on_stop, kind == "speed_cap", kind == "torque/reported", kind == "torque/solve"],
                    [0.0, s * vlim * u(0.998, 1.0), -s * vlim * u(0.1, 0.3), -s * vlim * u(0.5, 0.9)], u(-1.0, 1.0))    # the torque cells: moving AWAY from the target
    fa = np.select([kind == "on_stop/leaves", kind == "action_clip"], [-s * u(0.2, 1.0), s * u(1.05, 1.5)], s)

    o = make(cfg)
    created = o.get_state()

    def load(x, q_, qd_):
        x.set_state(created)
        x.dof_pos[:], x.dof_vel[:] = q_, qd_
        x.dof_pos[row[stop | on_stop], env[stop | on_stop]] = np.where(np.abs(q_[row, env] - L) < 1e-12, L32, x.dof_pos[row, env])[stop | on_stop]
        x.ball[0:3] = np.array([[10.0], [10.0], [5.0]])
        x.ball[7:13] = 0.0

    def actions_of(act_):
        return np.ascontiguousarray(act_.reshape(A, 7, n).transpose(2, 0, 1).reshape(n * A, 7), np.float32)

    # (1) the other joints of the envs that are to stay on the stop, and of those that are to exceed the speed cap
    stay, cap = stop | (kind == "on_stop/held"), kind == "speed_cap"
    uncapped = make(counterfactual_configs(cfg)["vel_limit"])
    best, best_score = (q, qd, act), np.full(n, -np.inf)
    for k in range(CANDIDATES):
        cq = q if k == 0 else np.clip(rng.uniform(lo[:, None], hi[:, None], (7 * A, n)), (lo + 0.01)[:, None], (hi - 0.01)[:, None])
        cqd = qd if k == 0 else u(-8.0, 8.0, (7 * A, n))
        ca = act if k == 0 else np.where(rng.random((7 * A, n)) < 0.5, to_act(cq), u(-1.0, 1.0, (7 * A, n)))
        cq, cqd, ca = cq.copy(), cqd.copy(), ca.copy()
        cq[row, env], cqd[row, env], ca[row, env] = np.where(cap, fq, L), np.where(cap, fqd, 0.0), s
        load(o, cq, cqd)
        score = np.zeros(n)
        for _ in range(STEPS):
            o.step(actions_of(ca))
            score += (o.dof_pos[row, env] == L32) & (o.dof_vel[row, env] == 0)
        load(uncapped, cq, cqd)
        uncapped.step(actions_of(ca))
        score = np.where(cap, s * uncapped.dof_vel[row, env], score)
        better = (stay | cap) & (score > best_score)
        best = tuple(np.where(better[None, :], c_, b_) for c_, b_ in zip((cq, cqd, ca), best))
        best_score = np.where(better, score, best_score)
    uncapped.close()
    q, qd, act = (np.array(x) for x in best)
    q[row, env], qd[row, env], act[row, env] = fq, fqd, fa

    # (2) the stops: the distance from what the joint travels
    v, f = u(3.0, 20.0), np.where(kind == "stop/substep0", u(0.1, 0.8), u(1.2, 1.8))
    wide, wide_first = make(widened(cfg)), make(first_substep_config(widened(cfg)))
    dist = np.full(n, 0.05)
    qd[row[stop], env[stop]] = (s * v)[stop]
    for _ in range(3):
        q[row[stop], env[stop]] = (L - s * dist)[stop]
        ends = []
        for x in (wide_first, wide):
            load(x, q, qd)
            start = np.array(x.dof_pos[row, env], np.float64)
            x.step(widened_actions(cfg, actions_of(act)))
            ends.append(np.array(x.dof_pos[row, env], np.float64))
        d1, d2 = s * (ends[0] - start), s * (ends[1] - ends[0])
        dist = np.where(f < 1.0, f * d1, d1 + (f - 1.0) * d2)
    reachable = stop & (d1 > 0) & ((f < 1.0) | (d2 > 0)) & (dist > 0)
    q[row[stop], env[stop]] = np.where(reachable, L - s * dist, L - s * 0.05)[stop]
    wide.close(); wide_first.close()
    load(o, q, qd)
    return o, actions_of(act), dict(joint=joint, arm=arm, row=row, sign=s, share=share, kind=kind, fraction=np.where(stop, f, np.nan), held_steps=best_score)


def counterfactual_configs(cfg):
    """{name: Config}.  Only the oracle is ever built from these."""
    out = {k: sc._copy(cfg) for k in ("effort", "vel_limit", "clip")}
    out["limits"] = widened(cfg)
    for j in range(7):
        out["effort"].joint[j].effort *= 100.0
        out["vel_limit"].joint[j].vel_limit *= 100.0
        out["clip"].clip_actions *= 100.0
    return out


def first_substep_config(cfg):
    """The oracle's first substep as a step of its own (h = dt / substeps is unchanged)."""
    c = sc._copy(cfg)
    assert cfg.substeps == 2
    c.substeps, c.dt = 1, cfg.dt / 2
    return c


def _focus(x, name, row):
    return getattr(x, name)[row, np.arange(len(row))].astype(np.float64)


def _beyond(a, b, name, row, factor, sign=None):
    """bool [n]: the focus joint's tensor `name` of oracle result a differs from b's by more than factor x the comparison tolerance (factor 0: at
    all); with sign [n], only where a lies beyond b on that side."""
    x, y = _focus(a, name, row), _focus(b, name, row)
    d = x - y if sign is None else (x - y) * sign
    return (np.abs(d) if sign is None else d) > factor * (RTOL * SCALES[name] + RTOL * np.abs(y))


def classify(cfg, meta, act, before, main, cf, first, gains):
    """-> {cell/sign: bool [n]} + {"cap_at_end/sign"} of one env-step.  before / main: snapshots of the stock oracle before / after it; cf[name]: of the
    counterfactual oracles after it; first: of the one-substep oracle; gains: (kp, kd) [7 A, n] of the envs."""
    n, A, J = len(meta["row"]), cfg.num_humanoids, joint_table(cfg)
    row, joint, env = meta["row"], meta["joint"], np.arange(n)
    f32 = lambda k: np.array([getattr(cfg.joint[j], k) for j in joint], np.float32)
    q0, v0 = before.dof_pos[row, env], before.dof_vel[row, env]
    q1, v1, tau1 = main.dof_pos[row, env], main.dof_vel[row, env], main.dof_force[row, env]
    a = act.reshape(n, A, 7)[env, meta["arm"], joint].astype(np.float64)
    clip = float(cfg.clip_actions)
    target = 0.5 * (f32("upper") + f32("lower")) + 0.5 * (f32("upper") - f32("lower")) * np.clip(a, -clip, clip).astype(np.float32)      # pd_target, fp32
    h = float(cfg.dt) / cfg.substeps
    kp, kd = gains[0][row, env], gains[1][row, env]
    tau0 = kp * (target.astype(np.float64) - q0 - h * v0) - kd * v0
    moved = {k: _beyond(cf[k], main, "dof_pos", row, REACHED) | _beyond(cf[k], main, "dof_vel", row, REACHED) for k in cf}
    c = {}
    for sign, name in ((1.0, "upper"), (-1.0, "lower")):
        L, vlim, eff = f32(name), np.float32(sign) * f32("vel_limit"), np.float32(sign) * f32("effort")
        early = first.dof_pos[row, env] == L
        c[f"stop/substep0/{name}"], c[f"stop/later/{name}"] = (q0 != L) & early & moved["limits"], (q0 != L) & ~early & (q1 == L) & moved["limits"]
        rest = (q0 == L) & (v0 == 0)
        c[f"ends_on_stop/{name}"] = (q1 == L) & (v1 == 0)
        c[f"on_stop/held/{name}"] = rest & (np.abs(target - L) <= 2 * np.spacing(np.abs(L))) & (q1 == L) & (v1 == 0) & ((_focus(cf["limits"], "dof_pos", row) - L) * sign > 0)
        c[f"on_stop/leaves/{name}"] = rest & (q1 != L) & (_beyond(main, before, "dof_pos", row, REACHED) | _beyond(main, before, "dof_vel", row, REACHED))
        faster = (_focus(cf["vel_limit"], "dof_vel", row) - _focus(main, "dof_vel", row)) * sign > 0
        c[f"speed_cap/{name}"] = moved["vel_limit"] & (faster | (v1 == vlim))
        c[f"cap_at_end/{name}"] = (v1 == vlim) & _beyond(cf["vel_limit"], main, "dof_vel", row, REACHED, sign)
        c[f"torque/solve/{name}"] = (tau0 * sign > f32("effort")) & moved["effort"]
        c[f"torque/reported/{name}"] = (tau1 == eff) & _beyond(cf["effort"], main, "dof_force", row, REACHED)
        c[f"torque_at_end/{name}"] = (tau1 == eff) & _beyond(cf["effort"], main, "dof_force", row, REACHED, sign)
        c[f"action_clip/{name}"] = (a * sign > clip) & (moved["clip"] | _beyond(cf["clip"], main, "dof_force", row, REACHED))
    return c


@functools.lru_cache(maxsize=None)
def oracle_run(variant, n, dr, seed=None):
    """The reference trajectory of a case: STEPS oracle steps.  -> namespace(cfg, probe, tables, steps, meta, excluded, resets, num_agents); a step is
    a dict: st (the oracle's state blob at its start), act, before / main (snapshots of the oracle before / after it), keep
    (~ SensitivityProbe.sensitive), cells (classify), edge (zeros: ball_contact_scenarios.compare_step's plain tolerances).  Computed once per case
    and shared; nothing in it is to be written to."""
    from oracle import binding
    binding.build()
    seed = seed_of(variant, n, dr) if seed is None else seed
    cfg = case_config(variant, n)
    A = cfg.num_humanoids
    tables = gain_tables(n, seed) if dr else None

    def make(c):
        x = binding.OracleEnv(c, threads=8)
        if dr:
            x.set_randomization(**tables, **NO_NOISE)
        return x
    first = make(first_substep_config(cfg))
    cf = {k: make(c) for k, c in counterfactual_configs(cfg).items()}
    probe = SensitivityProbe(binding, cfg)
    if dr:
        probe.o2.set_randomization(**tables, **NO_NOISE)
    J = joint_table(cfg)
    gains = tuple(np.tile(J[k], A)[:, None] * (np.tile(tables[t].astype(np.float64), (A, 1)) if dr else np.ones((7 * A, n)))
                  for k, t in (("kp", "dof_stiffness_scale"), ("kd", "dof_damping_scale")))
    o, act, meta = start_state(make, cfg, n, np.random.default_rng([seed, 5]))
    steps, excluded, resets = [], 0, 0
    for t in range(STEPS):
        st, before = o.get_state(), sc.snapshot(o)
        o.step(act)
        main = sc.snapshot(o)
        resets += int(main.reset_buf.sum())
        others = {}
        for k, x in list(cf.items()) + [("first", first)]:
            x.set_state(st)
            x.step(widened_actions(cfg, act) if k == "limits" else act)
            others[k] = sc.snapshot(x)
        keep = ~probe.sensitive(st, act, o)
        excluded += int((~keep).sum())
        cells = classify(cfg, meta, act, before, main, {k: others[k] for k in cf}, others["first"], gains)
        steps.append(dict(st=st, act=act, before=before, main=main, keep=keep, cells=cells, edge=np.zeros(n), cf=others))
    for x in list(cf.values()) + [first]:
        x.close()
    return types.SimpleNamespace(cfg=cfg, probe=probe, tables=tables, gains=gains, steps=steps, meta=meta, excluded=excluded, resets=resets, num_agents=A)


def gain_dependence(run):
    """-> (env-steps whose focus joint's explicit torque at the step's start is beyond +-effort under the env's own kp / kd and within it under the
    config's, env-steps the other way round): from the tables, the config and the oracle's tensors before the step, in fp64."""
    cfg, m = run.cfg, run.meta
    J, n, A = joint_table(cfg), len(m["row"]), run.num_agents
    env, h, clip = np.arange(n), float(cfg.dt) / cfg.substeps, float(cfg.clip_actions)
    only, ceases = 0, 0
    for s in run.steps:
        q0, v0 = (getattr(s["before"], k)[m["row"], env].astype(np.float64) for k in ("dof_pos", "dof_vel"))
        a = np.clip(s["act"].reshape(n, A, 7)[env, m["arm"], m["joint"]].astype(np.float64), -clip, clip)
        target = 0.5 * (J["upper"] + J["lower"])[m["joint"]] + 0.5 * (J["upper"] - J["lower"])[m["joint"]] * a
        tau = lambda kp, kd: np.abs(kp * (target - q0 - h * v0) - kd * v0) > J["effort"][m["joint"]]
        own, stock = tau(run.gains[0][m["row"], env], run.gains[1][m["row"], env]), tau(J["kp"][m["joint"]], J["kd"][m["joint"]])
        only, ceases = only + int((own & ~stock).sum()), ceases + int((~own & stock).sum())
    return only, ceases


def cell_counts(run, kept=True):
    """-> {cell/sign: kept env-steps per joint [7]} (T4: over both arms), {cell/sign: per (arm, joint) [A, 7]}."""
    A = run.num_agents
    per = {k: np.zeros((A, 7), np.int64) for k in run.steps[0]["cells"]}
    for s in run.steps:
        for name, mask in s["cells"].items():
            m = mask & (s["keep"] | (not kept))
            np.add.at(per[name], (run.meta["arm"][m], run.meta["joint"][m]), 1)
    return {k: v.sum(axis=0) for k, v in per.items()}, per


def assert_floor(run, what):
    counts, per = cell_counts(run)
    before, _ = cell_counts(run, kept=False)
    for name in CELLS + tuple(f"{x}/{s}" for x in EXTRA for s in SIGNS):
        print(f"{what} {name:24s} kept per joint {counts[name].tolist()} of {before[name].tolist()}")
    low = {k: counts[k].tolist() for k in CELLS if counts[k].min() < FLOOR}
    assert not low, f"{what}: (joint, cell, sign) under the floor of {FLOOR} kept env-steps: {low}"
    idle = {k: per[k].tolist() for k in CELLS if per[k].min() < 1}
    assert not idle, f"{what}: an arm that never reaches a (joint, cell, sign): {idle}"


def assert_cap(run, what):
    total = run.steps[0]["keep"].size * STEPS
    print(f"{what}: SensitivityProbe set aside {run.excluded} of {total} env-steps ({100 * run.excluded / total:.3f} %)")
    assert run.excluded <= EXCLUDED_CAP * total, what
    assert run.resets == 0, f"{what}: {run.resets} resets"


EXTRA = ("ends_on_stop", "cap_at_end", "torque_at_end")     # classify's keys beside CELLS: where an end-of-step value is exact (exact_masks)


def exact_masks(s):
    """-> {tensor: bool [n]}: the kept env-steps of step dict `s` on which the focus joint's dof_pos / dof_vel / dof_force must equal the oracle's fp32
    value bit for bit.  dof_pos = float32(limit) and dof_vel = 0 in the cells stop/*, on_stop/held where the oracle ENDS the step on the stop at
    rest (a stop taken in substep 0 may be left in substep 1, and then nothing is exact); dof_vel = +-float32(vel_limit) where the oracle ends at
    the cap and counterfactual (b) ends beyond it by REACHED x the tolerance; dof_force = +-float32(effort) where the oracle reports it and
    counterfactual (a) reports REACHED x the tolerance more."""
    c = s["cells"]
    stop = np.any([c[f"{x}/{sg}"] & c[f"ends_on_stop/{sg}"] for x in EXACT_CELLS for sg in SIGNS], axis=0) & s["keep"]
    cap = np.any([c[f"speed_cap/{sg}"] & c[f"cap_at_end/{sg}"] for sg in SIGNS], axis=0) & s["keep"]
    return dict(dof_pos=stop, dof_vel=stop | cap, dof_force=np.any([c[f"torque_at_end/{sg}"] for sg in SIGNS], axis=0) & s["keep"])


def assert_exact(got, s, meta, what):
    """The exactness assertion of a kernel's step (state view `got`) against the oracle's."""
    env = np.arange(len(meta["row"]))
    for name, m in exact_masks(s).items():
        g, w = getattr(got, name)[meta["row"], env][m], getattr(s["main"], name)[meta["row"], env][m]
        bad = np.ascontiguousarray(g, np.float32).view(np.uint32) != np.ascontiguousarray(w, np.float32).view(np.uint32)
        assert not bad.any(), f"{what}: {name} of the focus joint is not the oracle's fp32 value bit for bit in envs {np.flatnonzero(m)[bad][:8]}: {g[bad][:8]} against {w[bad][:8]}"
    return {k: int(v.sum()) for k, v in exact_masks(s).items()}
