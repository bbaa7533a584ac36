"""Scripted states that put the 27-dof tree on every regime of joint_torque (csrc/ppenv_ta_device.h): the limit spring's quadratic toe below
0.01 rad and its linear law beyond, both signs, its damper on the same ramp with the joint moving out and moving in, the speed-cap damper whose
implicit term fades in over 1 rad/s and the full one beyond, both at once, and the drive's effort clamp before the solve and in the reported
dof_force — and the oracle-only book-keeping of the tests that use them (tests/test_ta_joint_limits_host.py / _gpu.py).

The free-running rollouts meet these regimes a handful of times on most joints and never on some; the scripted 27-dof suites clip
their poses 0.01 rad inside the limits or stand at rest.  Here every env is a humanoid in the standing pose, its root placed as
ta_ball_contact_scenarios places a resting one (displaced by up to 0.1 m, turned by up to 0.4 rad about z), the ball far away at (10, 10, 5)
flying at 3 m/s along x, with ONE focus joint env % 27 and a case (cell, sign) that cycles with env // 27 (CASES: weighted by what an env yields); the
actions hold the drawn pose (ta_branch_scenarios.hold_actions' rule:
the target is the pose, clipped into the limits), except in the torque cases, whose target is the far stop.  STEPS steps, each restarted from the
oracle's tensors, actions held.

Everything is decided from the ORACLE and the model, never from a kernel's output.  An env-step's cells (of its focus joint; sign "upper" = beyond
the upper limit / qd > 0 / torque > 0) are read off the oracle's tensors at the step's START — over = q - upper or q - lower, ex = |qd| -
vel_limit — and off counterfactual oracles stepped from the same state whose model has (a) limit_stiffness = limit_damping = 0, (b)
vel_limit_damping = 0, (c) every effort x 100; "reached" means that the focus joint's q, qd or dof_force of that counterfactual differs from the
stock oracle's by at least REACHED x check_step's tolerance:
  limit/toe              0 < |over| < 0.01 (any qd); counted where (a) is reached (classify's key toe_reached), see reached_joints
  limit/toe_moving_out   the toe with |qd| >= 1 rad/s away from the range, (a) reached: the damper term ramp * c_lim * qd
  limit/toe_moving_in    the same, moving back into the range
  limit/linear           |over| >= 0.01, ex <= 0, (a) reached
  speed_cap/fade_in      over == 0, 0 < ex < 1, (b) reached
  speed_cap/full         over == 0, ex >= 1, (b) reached
  both                   over != 0 and ex > 0, (a) and (b) reached
  torque/solve           kp (err - h qd) - kd qd at the step's start (fp64, from the tensors and the model) beyond +-effort, (c) reached in q or qd
  torque/reported        dof_force == +-float32(effort) after the step, (c) reached in dof_force
The toe's spring torque is at most k_lim x 0.01^2 x 50 = 0.1 N m, and the fading-in damper acts on less than 1 rad/s for one substep: the floor of
these two WEAK_CELLS is asserted over the joints on which the oracle shows them reached (assert_floor prints them; at REACHED the toe is reached on
all 27, the fade-in on all but the waist roll and the wrists' last joints), which must include one of every limb; the others are compared, not
counted.  The ankle rolls and the left ankle pitch (kp x range + (kd + kp h) x vel_limit < 1.5 x effort) cannot saturate their drive from any state
the draws allow: torque_joints leaves them out of the two torque cells, by the model's numbers alone."""
import functools
import types

import numpy as np

import ta_branch_scenarios as tb
from ball_contact_scenarios import REACHED as REACHED_7DOF
from helpers import RTOL
from isaacgym_amd import scene
from ta_ball_contact_scenarios import _axis_angle, _quat_mul

STEPS = 3
FLOOR = 8
ENV_SEED = tb.ENV_SEED
EXCLUDED_BOUND = tb.EXCLUDED_BOUND
# "Reached" = 10 x check_step's tolerance, a tenth of the 7-dof suites' factor: TOL["qd"] = 5e-4 x 40 rad/s is 22 x the 7-dof dof_vel tolerance
# (1e-4 x 0.25 x 37), so 10 x TOL["qd"] = 0.2 rad/s still asks for twice the 0.09 rad/s that REACHED asks of an arm joint, while 100 x would ask a leg
# of 0.6 kg m^2 for 2 rad/s in one step: 145 N m, more than the limit spring gives anywhere in the 0.08 rad the cells reach.  A kernel that drops
# the term is 10 x outside what check_step admits; the kernels' own error on these states is below 0.1 x the tolerance.
REACHED = REACHED_7DOF / 10.0
CELL_NAMES = ("limit/toe", "limit/toe_moving_out", "limit/toe_moving_in", "limit/linear", "speed_cap/fade_in", "speed_cap/full", "both",
              "torque/solve", "torque/reported")
SIGNS = ("upper", "lower")
CELLS = tuple(f"{c}/{s}" for c in CELL_NAMES for s in SIGNS)
# Shares of a cell in the cycle of cases, from what one env yields: a toe env is pushed out of the toe within a step, a joint moving back in leaves
# it sooner still, and above the speed cap the damper acts in the first substep only, so that on the heavier joints few of the drawn excesses move the
# end of the step by REACHED x the tolerance.
SHARES = {"limit/toe": 2, "limit/toe_moving_out": 3, "limit/toe_moving_in": 9, "limit/linear": 1, "speed_cap/fade_in": 4, "speed_cap/full": 6, "both": 4,
          "torque/solve": 1, "torque/reported": 3}
CASES = tuple((c, s) for c in CELL_NAMES for _ in range(SHARES[c]) for s in (1.0, -1.0))
COUNTED = 3 * 27 * len(CASES)          # 5346: three whole cycles, ragged (83 workgroups of 64 and 34 envs)
LIMBS = dict(left_leg=range(0, 6), right_leg=range(6, 12), waist=range(12, 15), left_arm=range(15, 22), right_arm=range(22, 27))


def joint_table(m):
    return {k: np.array([getattr(m.link[i], k) for i in range(1, 28)], np.float64) for k in ("lower", "upper", "kp", "kd", "effort", "vel_limit")}


def torque_joints(cfg, m):
    """The joints whose drive CAN saturate: kp x range + (kd + kp h) x vel_limit, the explicit torque of a joint at one stop moving at its speed
    cap away from a target on the other, exceeds 1.5 x effort.  -> bool [27]"""
    J, h = joint_table(m), float(cfg.dt) / cfg.substeps
    return J["kp"] * (J["upper"] - J["lower"]) + (J["kd"] + J["kp"] * h) * J["vel_limit"] > 1.5 * J["effort"]


def scenarios(n, seed):
    """-> root [n,3,13], dof [n,27,2], progress [n], actions [n,27] (held), meta (joint, sign, kind [n])."""
    p, cfg, m = scene.build_ta_params(n), scene.build_ta_scene(n), scene.build_ta_model()
    rng = np.random.default_rng(seed)
    u = lambda lo_, hi_: rng.uniform(lo_, hi_, n)
    J = joint_table(m)
    env = np.arange(n)
    joint, case = env % 27, (env // 27) % len(CASES)
    kind, s = np.array([c for c, _ in CASES])[case], np.array([x for _, x in CASES])[case]
    L, Lopp = np.where(s > 0, J["upper"][joint], J["lower"][joint]), np.where(s > 0, J["lower"][joint], J["upper"][joint])
    vlim, span = J["vel_limit"][joint], (J["upper"] - J["lower"])[joint]

    root = np.zeros((n, 3, 13), np.float64)
    for a in range(3):
        root[:, a, :7] = np.array(list(p.init_root[a]))
    root[:, 0, 0:2] += rng.uniform(-0.1, 0.1, (n, 2))
    root[:, 0, 3:7] = _quat_mul(_axis_angle(np.tile([0.0, 0, 1.0], (n, 1)), u(-0.4, 0.4)), root[:, 0, 3:7])
    root[:, 2, 0:3] = np.array([10.0, 10.0, 5.0])
    root[:, 2, 7] = 3.0                                       # (vx = 0 is a branch threshold of the reward: near_threshold would set every env aside)
    q = np.tile(np.array(list(p.init_dof_pos), np.float64), (n, 1))
    qd = np.zeros((n, 27))
    inside = L - s * np.minimum(0.3, 0.4 * span)               # speed cases: inside the range, moving towards the stop of the sign
    toe, moving = np.isin(kind, ("limit/toe", "limit/toe_moving_out", "limit/toe_moving_in")), np.isin(kind, ("limit/toe_moving_out", "limit/toe_moving_in"))
    torque = np.isin(kind, ("torque/solve", "torque/reported"))
    fq = np.select([toe, kind == "limit/linear", kind == "both", torque], [L + s * u(0.001, 0.009), L + s * u(0.012, 0.08), L + s * u(0.002, 0.05), Lopp + s * u(0.0, 0.3) * span],
                   inside)
    ex = np.select([kind == "speed_cap/fade_in", kind == "speed_cap/full"], [u(0.05, 0.9), u(1.1, 5.0)], u(0.05, 5.0))
    fqd = np.select([moving, np.isin(kind, ("speed_cap/fade_in", "speed_cap/full", "both")), torque],
                    [np.where(kind == "limit/toe_moving_out", s, -s) * u(1.0, 4.0), s * (vlim + ex), -s * vlim * u(0.2, 0.8)], 0.0)
    q[env, joint], qd[env, joint] = fq, fqd
    hold = np.clip((q - 0.5 * (J["upper"] + J["lower"])) / (0.5 * (J["upper"] - J["lower"])), -1.0, 1.0)
    hold[env[torque], joint[torque]] = s[torque]              # the torque cases: the target on the far stop, the joint moving away from it
    dof = np.ascontiguousarray(np.stack([q, qd], axis=2), np.float32)
    progress = rng.integers(0, p.max_episode_length - 1 - STEPS, n).astype(np.int64)      # nobody times out inside the run
    return root.astype(np.float32), dof, progress, np.ascontiguousarray(hold, np.float32), dict(joint=joint, sign=s, kind=kind)


def gain_tables(n, seed):
    """The randomised run: per-env kp / kd scales of every joint (the gains move the saturation point; limits, masses and materials stay)."""
    rng = np.random.default_rng([seed, 79])
    return dict(dof_stiffness_scale=rng.uniform(0.5, 1.5, (27, n)).astype(np.float32), dof_damping_scale=rng.uniform(0.5, 1.5, (27, n)).astype(np.float32))


def counterfactual_models(m):
    """{name: model}.  Only the oracle is ever stepped with these."""
    copy = lambda: type(m).from_buffer_copy(m)
    out = {"limit": copy(), "vel": copy(), "effort": copy()}
    out["limit"].limit_stiffness = out["limit"].limit_damping = 0.0
    out["vel"].vel_limit_damping = 0.0
    for i in range(1, 28):
        out["effort"].link[i].effort *= 100.0
    return out


def _differs(a, b, tol, factor):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) > factor * (tol + RTOL * np.abs(b.astype(np.float64)))      # assert_close's form


def classify(cfg, m, meta, s, cf, tables=None):
    """-> {cell/sign: bool [n]} of step dict `s` (root0, dof0, act, after_sim); cf[name] = (dof, frc) of the counterfactual oracles after the step;
    tables: the run's gain tables (the explicit torque at the step's start is the env's own)."""
    import test_ta_physics as tp
    J, joint = joint_table(m), meta["joint"]
    n = len(joint)
    env, h = np.arange(n), float(cfg.dt) / cfg.substeps
    q0, v0 = s["dof0"][env, joint, 0].astype(np.float64), s["dof0"][env, joint, 1].astype(np.float64)
    dof1, frc1 = s["after_sim"][1], s["after_sim"][3]
    lo, hi, eff = (np.array([getattr(m.link[j + 1], k) for j in joint], np.float32) for k in ("lower", "upper", "effort"))
    over = np.where(q0 > hi, q0 - hi, np.where(q0 < lo, q0 - lo, 0.0))
    ex = np.abs(v0) - J["vel_limit"][joint]
    moved, force = {}, {}
    for k, (dof_c, frc_c) in cf.items():
        moved[k] = _differs(dof_c[env, joint, 0], dof1[env, joint, 0], tp.TOL["q"], REACHED) | _differs(dof_c[env, joint, 1], dof1[env, joint, 1], tp.TOL["qd"], REACHED)
        force[k] = _differs(frc_c[env, joint], frc1[env, joint], tp.TOL["frc"], REACHED)
    clip = float(cfg.clip_actions)
    target = 0.5 * (J["upper"] + J["lower"])[joint] + 0.5 * (J["upper"] - J["lower"])[joint] * np.clip(s["act"][env, joint].astype(np.float64), -clip, clip)
    kp, kd = (J[k][joint] * (tables[t][joint, env].astype(np.float64) if tables else 1.0) for k, t in (("kp", "dof_stiffness_scale"), ("kd", "dof_damping_scale")))
    tau0 = kp * (target - q0 - h * v0) - kd * v0
    c = {}
    for sign, name in ((1.0, "upper"), (-1.0, "lower")):
        out, toe = over * sign > 0, (over * sign > 0) & (np.abs(over) < 0.01)
        any_a = moved["limit"] | force["limit"]
        c[f"limit/toe/{name}"] = toe
        c[f"toe_reached/{name}"] = toe & any_a
        c[f"limit/toe_moving_out/{name}"] = toe & (v0 * sign >= 1.0) & any_a
        c[f"limit/toe_moving_in/{name}"] = toe & (v0 * sign <= -1.0) & any_a
        c[f"limit/linear/{name}"] = out & (np.abs(over) >= 0.01) & (ex <= 0) & any_a
        fast = (v0 * sign > 0) & (ex > 0) & (moved["vel"] | force["vel"])
        c[f"speed_cap/fade_in/{name}"], c[f"speed_cap/full/{name}"] = fast & (over == 0) & (ex < 1.0), fast & (over == 0) & (ex >= 1.0)
        c[f"both/{name}"] = fast & out & any_a
        c[f"torque/solve/{name}"] = (tau0 * sign > eff) & moved["effort"]
        c[f"torque/reported/{name}"] = (frc1[env, joint] == np.float32(sign) * eff) & force["effort"]
    return c


@functools.lru_cache(maxsize=None)
def oracle_run(n, seed, dr=False, per_env_irb=False):
    """The reference trajectory of `scenarios(n, seed)`: STEPS steps of the oracle's rigid-body step + post_physics_step; dr: every oracle involved
    steps with gain_tables (ta_simulate_dr).  -> namespace(p, irb, tables, steps, meta, cfg, m); a step is ta_branch_scenarios.oracle_run's dict (root0, dof0, flags0, episode0, progress0, act, after_sim, main, switch, near,
    cells) plus edge (zeros: ta_ball_contact_scenarios.compare_step's plain tolerances).  Computed once per key and shared; nothing in it is to be
    written to."""
    import ta_ball_contact_scenarios as bc
    import test_ta_physics as tp
    from oracle import binding
    binding.build()
    cfg, m, p = scene.build_ta_scene(n), scene.build_ta_model(), scene.build_ta_params(n, seed=ENV_SEED)
    root, dof, progress, act, meta = scenarios(n, seed)
    tables = gain_tables(n, seed) if dr else None
    stand = np.zeros((1, 3, 13), np.float32)
    for a in range(3):
        stand[0, a, :7] = np.array(list(p.init_root[a]))
    irb = binding.ta_forward_kinematics(m, stand, np.zeros((1, 27, 2), np.float32))       # TA:1152 initial_body_states
    p.initial_rb_shared = 0 if per_env_irb else 1
    if per_env_irb:
        irb = np.ascontiguousarray(np.broadcast_to(irb, (n, 42, 13)))
    cfm = counterfactual_models(m)
    flags, episode = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    steps = []
    for t in range(STEPS):
        s = dict(root0=root.copy(), dof0=dof.copy(), flags0=flags.copy(), episode0=episode.copy(), progress0=progress.copy(), act=act, edge=np.zeros(n))
        make = lambda model: bc.simulator(binding, cfg, model, tables, p.seed, p.env_id_offset, s["episode0"], s["progress0"])
        cf = {}
        for k, mk in cfm.items():
            r2, d2 = s["root0"].copy(), s["dof0"].copy()
            cf[k] = (d2, make(mk)(act, r2, d2)[1])
        rb, frc, pvx = make(m)(act, root, dof)
        s["after_sim"] = (root.copy(), dof.copy(), rb, frc, pvx)
        s["switch"] = bc.switch_probe(binding, cfg, m, make(m) if dr else None, s, seed=300 + t)
        s["near"] = tb.near_threshold(s["flags0"], root, rb, irb, tp.TOL["root_pos"], tp.TOL["rb_pos"], tp.TOL["root_vel"])
        s["cells"] = classify(cfg, m, meta, s, cf, tables)
        obs, rew, reset = binding.ta_post_physics_step(p, rb, irb, root, dof, frc, pvx, None, flags, episode, progress)
        s["main"] = (root.copy(), dof.copy(), rb, frc, obs, rew, reset, progress.copy(), episode.copy(), flags.copy())
        steps.append(s)
    return types.SimpleNamespace(p=p, irb=irb, tables=tables, steps=steps, meta=meta, cfg=cfg, m=m)


def gain_dependence(run):
    """-> (env-steps whose focus joint's explicit torque at the step's start is beyond +-effort under the env's own kp / kd and within it under the
    model's, env-steps the other way round): from the tables, the model and the oracle's tensors at the step's start, in fp64."""
    J, joint, n = joint_table(run.m), run.meta["joint"], len(run.meta["joint"])
    env, h, clip = np.arange(n), float(run.cfg.dt) / run.cfg.substeps, float(run.cfg.clip_actions)
    only, ceases = 0, 0
    for s in run.steps:
        q0, v0 = s["dof0"][env, joint, 0].astype(np.float64), s["dof0"][env, joint, 1].astype(np.float64)
        target = 0.5 * (J["upper"] + J["lower"])[joint] + 0.5 * (J["upper"] - J["lower"])[joint] * np.clip(s["act"][env, joint].astype(np.float64), -clip, clip)
        tau = lambda ks, ds: np.abs(J["kp"][joint] * ks * (target - q0 - h * v0) - J["kd"][joint] * ds * v0) > J["effort"][joint]
        own, stock = tau(run.tables["dof_stiffness_scale"][joint, env], run.tables["dof_damping_scale"][joint, env]), tau(1.0, 1.0)
        only, ceases = only + int((own & ~stock).sum()), ceases + int((~own & stock).sum())
    return only, ceases


def cell_counts(run, kept=True):
    """-> {cell/sign: kept env-steps per joint [27]}."""
    counts = {k: np.zeros(27, np.int64) for k in run.steps[0]["cells"]}
    for s in run.steps:
        k = ~(s["switch"] | s["near"]) if kept else np.ones(len(run.meta["joint"]), bool)
        for name, mask in s["cells"].items():
            np.add.at(counts[name], run.meta["joint"][mask & k], 1)
    return counts


WEAK_CELLS = {"limit/toe": "toe_reached", "speed_cap/fade_in": "speed_cap/fade_in"}     # cell: the key of classify that holds its REACHED env-steps


def reached_joints(run, cell):
    """The joints on which the oracle shows a weak cell REACHED (its counterfactual differs by REACHED x the tolerance) in at least FLOOR kept
    env-steps of either sign: the joints that cell's floor is asserted over.  -> bool [27]"""
    counts = cell_counts(run)
    return np.all([counts[f"{WEAK_CELLS[cell]}/{sg}"] >= FLOOR for sg in SIGNS], axis=0)


def assert_floor(run, what):
    """The floor over every (joint, cell, sign) — but for the two weak cells over the joints on which the oracle shows them reached (the toe's torque
    is at most 0.1 N m; the fading-in damper takes a fraction of an excess below 1 rad/s out of the first substep only, which on the waist roll
    and the wrists' last joints moves the end of the step by less than REACHED x the tolerance whatever the excess), which must include a joint of
    every limb and, for the fade-in, 20 of the 27 joints; and for the torque cells over the joints whose drive can saturate."""
    counts, before = cell_counts(run), cell_counts(run, kept=False)
    can = torque_joints(run.cfg, run.m)
    weak = {cell: reached_joints(run, cell) for cell in WEAK_CELLS}
    print(f"{what}: the drive can saturate on joints {np.flatnonzero(can).tolist()}")
    for cell, js_ in weak.items():
        print(f"{what}: {cell} is reached on joints {np.flatnonzero(js_).tolist()}; compared, not counted, on {np.flatnonzero(~js_).tolist()}")
    low = {}
    for name in CELLS:
        print(f"{what} {name:28s} kept per joint {counts[name].tolist()} (set aside {int((before[name] - counts[name]).sum())})")
        cell, sg = name.rsplit("/", 1)
        c = counts[f"{WEAK_CELLS[cell]}/{sg}"] if cell in WEAK_CELLS else counts[name]
        over = weak[cell] if cell in WEAK_CELLS else (can if cell.startswith("torque/") else np.ones(27, bool))
        if (c[over] < FLOOR).any():
            low[name] = c.tolist()
    assert not low, f"{what}: (joint, cell, sign) under the floor of {FLOOR} kept env-steps: {low}"
    for cell, js_ in weak.items():
        for limb, joints in LIMBS.items():
            assert js_[list(joints)].any(), f"{what}: {cell} is reached on no joint of the {limb}"
    assert weak["speed_cap/fade_in"].sum() >= 20 and can.sum() >= 24


def assert_excluded_share(run, what):
    n = len(run.meta["joint"])
    aside = sum(int((s["switch"] | s["near"]).sum()) for s in run.steps)
    near, switch = sum(int(s["near"].sum()) for s in run.steps), sum(int(s["switch"].sum()) for s in run.steps)
    print(f"{what}: set aside {aside} of {n * STEPS} env-steps ({100 * aside / (n * STEPS):.3f} %): {near} near a threshold, {switch} on a switch")
    assert aside <= EXCLUDED_BOUND * n * STEPS
    assert all(int(s["main"][6].sum()) == 0 for s in run.steps), f"{what}: somebody resets"
