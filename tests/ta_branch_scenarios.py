"""Scripted states that put the 27-dof task on every PAYING branch of compute_pingpong_reward_nv (TA:1440-1690), and the oracle-only
book-keeping of the tests that use them (tests/test_ta_reward_branches_host.py / _gpu.py).

The free-running parity rollouts of tests/test_ta_physics.py never bring the ball to the paddle, the net, the table or below it: only
the gated-off side of those branches is compared there.  `scenarios` starts every env from the task's standing pose and overwrites it by
group (env % 5): paddle, net, table, below, humanoid displaced.  The ball is AIMED: it flies freely (semi-implicit Euler, no drag:
`launch`) to a drawn place at a drawn step, step = (env % 7) % 3.  In the reset pass the envs with env % 7 = 0 / 1 / 2 time out in step
0 / 1 / 2 — every 7th env in each step — so an env's paying branch and its reset fall into the same step.  Inside a (group, env % 7) class
the case (which side of a threshold, which gate closed) cycles with the env's index, so that every cell of `CELLS` is reached by its
share of the envs whatever the seed; the sticky bits a case does not fix are drawn independently with probability 1/2.
(The humanoid here stands at rest: ball contacts with a MOVING humanoid are the suite of tests/ta_ball_contact_scenarios.py.)

Everything here is decided from the ORACLE's tensors: `classify` (which cells an env-step is in), `near_threshold` (which env-steps lie
within the comparison tolerance of a branch threshold and are set aside, as ball_switch_probe sets aside the contact switches) and
`oracle_run` (the reference trajectory, computed once per (n, seed, resets) and shared by the tests)."""
import functools

import numpy as np

from isaacgym_amd import scene

PADDLE_BODY = 39
STEPS = 3
FLOOR = 8                    # kept env-steps every cell must reach (per pass; the reset pass counts the env-steps that reset)
ENV_SEED = 11                # the task seed (the keyed reset draws) of the oracle's params and of the TAEnv under test
EXCLUDED_BOUND = 0.02        # scripted states sit near thresholds far more often than rollouts do (whose bound is 0.5 %)
PC, HTC, DPC, HD = scene.TA_FLAG_PADDLE_COND, scene.TA_FLAG_HIT_TABLE_CALC, scene.TA_FLAG_DIE_PENALTY_CALC, scene.TA_FLAG_HUMANOID_DIE_CALC
COUNT_BITS = dict(CLOSER=16, HIT_PADDLE=32, CROSS_NET=64, HIT_TABLE=128, FALL_DOWN=256)       # include/ppenv.h PPENV_TA_COUNT_*
STICKY_BITS = dict(PADDLE_COND=PC, HIT_TABLE_CALC=HTC, DIE_PENALTY_CALC=DPC, HUMANOID_DIE_CALC=HD)
BAL_IDS = [0, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25, 26, 27]   # yaml:57, the bodies of has_fallen

CELLS = (
    ["first_close/in_circle/hum_die_off", "first_close/in_circle/hum_die_on", "first_close/miss/hum_die_off", "first_close/miss/hum_die_on",
     "x_close/paddle_cond_set", "hit_paddle/paid", "hit_paddle/gated_paddle_cond", "hit_paddle/gated_hum_die"] +
    [f"z_in/{r}/{g}" for r in ("in_range", "out_of_range") for g in ("paid", "gated_hit_table_calc", "gated_hum_die")] +
    [f"over_net/{h}/{g}" for h in ("suitable", "too_high", "too_low") for g in ("hum_die_off", "hum_die_on")] +
    ["below/paid", "below/gated", "has_fallen/true", "has_fallen/false", "pelvis_low/true", "pelvis_low/false", "time_penalty/on", "time_penalty/off"])


def launch(cfg, target, vel, k):
    """Where a ball with velocity `vel` [..., 3] must start to be at `target` [..., 3] after k [...] free steps of the oracle's ball
    integrator (v.z += g hb, then p += v hb, substeps x ball_substeps times a step)."""
    per = cfg.substeps * cfg.ball_substeps
    hb = float(cfg.dt) / per
    m = np.asarray(k, np.float64) * per
    start = np.asarray(target, np.float64) - np.asarray(vel, np.float64) * (m * hb)[..., None]
    start[..., 2] -= float(cfg.gravity_z) * hb * hb * m * (m + 1) / 2
    return start


def hold_actions(model):
    """The actions whose PD targets (TA:1131: mid-range + half-range x action) are the standing pose's zero angles."""
    lo = np.array([model.link[i].lower for i in range(1, 28)])
    hi = np.array([model.link[i].upper for i in range(1, 28)])
    return np.clip(-(hi + lo) / (hi - lo), -1.0, 1.0)


def scenarios(n, seed, resets=False):
    """-> root [n,3,13], dof [n,27,2], flags [n] uint32, progress [n] int64, actions [n,27] (held over the STEPS steps).
    resets: the envs with env % 7 = 0 / 1 / 2 are 2 / 3 / 4 steps short of the time-out (they reset in step 0 / 1 / 2); the states are
    the same as without."""
    from oracle import binding
    binding.build()
    p, cfg, m = scene.build_ta_params(n), scene.build_ta_scene(n), scene.build_ta_model()
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    T = float(cfg.dt)
    root = np.zeros((n, 3, 13), np.float64)
    for a in range(3):
        root[:, a, :7] = np.array(list(p.init_root[a]))
    dof = np.zeros((n, 27, 2), np.float32)
    dof[:, :, 0], dof[:, :, 1] = np.array(list(p.init_dof_pos)), np.array(list(p.init_dof_vel))
    paddle = binding.ta_forward_kinematics(m, root[:1].astype(np.float32), dof[:1])[0, PADDLE_BODY, :3].astype(np.float64)

    env = np.arange(n)
    group, when, case = env % 5, (env % 7) % 3, env // 35
    bits = rng.integers(0, 2, (n, 4)).astype(bool)            # PADDLE_COND, HIT_TABLE_CALC, DIE_PENALTY_CALC, HUMANOID_DIE_CALC
    pos, vel = np.zeros((n, 3)), np.zeros((n, 3))
    flight = np.zeros(n)                                      # free steps before the ball is at `pos`

    # ---- paddle.  In the standing pose the blade (radius 0.075, centre = body 39) stands edge-on to x, its axis along y: a ball flying in
    #      -x at the blade's y and height bounces off its rim.  PADDLE_COND is set as soon as the ball is within 0.2 in x, a step's flight is
    #      at most 0.07: a bounce with the bit still clear (hit_paddle paid / gated by hum_die alone) can only be the scenario's FIRST step.
    #      Step 0: 12 + 12 + 2 towards the rim (paid / gated by hum_die / gated by paddle_cond), 1 + 1 past the blade outside the circle.
    #      Steps 1, 2: 8 towards the rim (paddle_cond set), 5 + 5 that ENTER the 0.2 band in that step inside the circle, beside the blade,
    #      5 + 5 outside it (hum_die off / on each).  kind: 0 - 2 rim, 3 / 4 inside, 5 / 6 outside.
    first = np.array([0, 1] * 12 + [2, 2, 5, 6])[case % 28]
    later = np.array([2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 2, 2, 2])[case % 28]
    kind = np.where(when == 0, first, later)
    g = group == 0
    vel[g] = np.stack([u(-8, -3), u(-0.1, 0.1), u(-0.1, 0.1)], axis=1)[g]
    travel = np.abs(vel[:, 0]) * T
    aim = g & (kind <= 2)          # at the START of step `when` less than a step's flight in front of the rim: the ball bounces in that step
    front = cfg.paddle_radius + cfg.ball_radius + u(0.1, 0.9) * travel
    pos[aim] = (paddle + np.stack([front, u(-0.004, 0.004), u(-0.02, 0.02)], axis=1))[aim]
    flight[aim] = when[aim]
    ang = u(0, 2 * np.pi)
    rad = np.where(kind <= 4, u(0.05, 0.145), np.where(rng.integers(0, 2, n) == 0, u(0.155, 0.2), u(0.2, 0.30)))   # half of the misses just outside 0.15
    miss = g & ~aim                # AFTER step `when` beside the blade and less than a step's flight inside the 0.2 band (step 0: anywhere in it)
    side = np.where(np.abs(np.cos(ang)) < 0.4, np.where(np.cos(ang) < 0, -0.4, 0.4), np.cos(ang))       # at least 0.02 from the blade's plane
    x = np.where(when == 0, u(-0.19, 0.19), 0.2 - u(0.05, 0.9) * travel)
    pos[miss] = (paddle + np.stack([x, rad * side, rad * np.sin(ang)], axis=1))[miss]
    flight[miss] = when[miss] + 1
    hd_off, hd_on = g & np.isin(kind, (0, 3, 5)), g & np.isin(kind, (1, 4, 6))
    bits[hd_off, 0], bits[hd_off, 3] = False, False
    bits[hd_on, 0], bits[hd_on, 3] = False, True
    bits[g & (kind == 2), 0] = True

    # ---- net: (suitable, too high, too low) x hum_die; a tenth of the x band lies outside 1.72 - 1.78; the net's top edge is at 0.9125
    g = group == 1
    kind = case % 6
    z = np.where(kind % 3 == 0, u(0.97, 1.24), np.where(kind % 3 == 1, u(1.255, 1.40), u(0.925, 0.958)))
    pos[g] = np.stack([u(1.717, 1.783), u(-0.7, 0.7), z], axis=1)[g]
    vel[g] = np.stack([u(2, 7), u(-1, 1), u(-1.5, 1.5)], axis=1)[g]
    flight[g] = when[g] + 1
    bits[g, 3] = (kind >= 3)[g]

    # ---- table: (in range, out of range) x (paid, gated by hit_table_calc, gated by hum_die); the last 5 of every 29 cases pass just outside the band 0.82 - 0.83
    g = group == 2
    kind = case % 6
    side = rng.integers(0, 3, n)
    x_out = np.where(side == 0, u(1.45, 1.72), np.where(side == 1, u(3.12, 3.4), u(1.9, 3.4)))      # (no flight through the net, which stands at 1.75)
    y_out = np.where(side == 2, u(0.62, 0.9) * rng.choice([-1.0, 1.0], n), u(-0.9, 0.9))
    inside = kind % 2 == 0
    z = np.where(case % 29 < 24, u(0.8205, 0.8295), np.where(rng.integers(0, 2, n) == 0, u(0.8165, 0.8195), u(0.8305, 0.8335)))
    pos[g] = np.stack([np.where(inside, u(1.92, 3.08), x_out), np.where(inside, u(-0.58, 0.58), y_out), z], axis=1)[g]
    vel[g] = np.stack([u(1, 5), u(-0.5, 0.5), u(-3, -1.3)], axis=1)[g]      # falls by more than the band's 0.01 a step: in the band once
    flight[g] = when[g] + 1
    gate = kind // 2
    bits[g & (gate == 0), 1], bits[g & (gate == 0), 3] = False, False
    bits[g & (gate == 1), 1] = True
    bits[g & (gate == 2), 1], bits[g & (gate == 2), 3] = False, True

    # ---- below: beyond the table's far end the ball falls through z = 0.78 in step `when` (or, in step 0, already lies 0.6 - 0.775);
    #      paid / gated by die_penalty_calc / gated by hum_die / stays above
    g = group == 3
    kind = case % 4
    vel[g] = np.stack([u(1, 4), u(-0.5, 0.5), u(-4, -1.5)], axis=1)[g]
    drop = np.abs(vel[:, 2]) * T
    z = 0.78 + np.where(kind == 3, u(1.3, 2.5), u(0.1, 0.8)) * drop
    z = np.where((when == 0) & (kind != 3) & (case % 8 < 4), u(0.6, 0.775), z)
    pos[g] = np.stack([u(3.2, 3.6), u(-0.7, 0.7), z], axis=1)[g]
    flight[g] = when[g]
    bits[g & (kind == 0), 2], bits[g & (kind == 0), 3] = False, False
    bits[g & (kind == 1), 2] = True
    bits[g & (kind == 2), 2], bits[g & (kind == 2), 3] = False, True

    # ---- humanoid displaced (has_fallen, pelvis_h < 0.97 each both ways), the ball in flight towards it
    g = group == 4
    root[g, 0, 0] += u(-0.6, 0.6)[g]
    root[g, 0, 2] += u(-0.3, 0.05)[g]
    pos[g] = np.stack([u(1.0, 2.5), u(-0.4, 0.1), u(1.0, 1.3)], axis=1)[g]
    vel[g] = np.stack([u(-6, -4), u(-0.5, 0.2), u(0.5, 2.0)], axis=1)[g]

    root[:, 2, 0:3] = launch(cfg, pos, vel, flight)
    root[:, 2, 7:10] = vel
    flags = (bits * np.array([PC, HTC, DPC, HD])).sum(axis=1).astype(np.uint32)
    progress = rng.integers(0, p.max_episode_length - 1 - STEPS, n).astype(np.int64)      # nobody times out inside the run
    if resets:
        for r in range(STEPS):
            progress[env % 7 == r] = p.max_episode_length - 2 - r
    actions = hold_actions(m) + rng.normal(0.0, 0.05, (n, 27))
    actions[group == 4] = rng.uniform(-1.0, 1.0, (n, 27))[group == 4]
    return root.astype(np.float32), dof, flags, progress, np.ascontiguousarray(actions, np.float32)


def _terms(flags0, root, rb, irb):
    """The quantities the branches compare, in fp64 from the oracle's post-simulate (pre-reset) tensors."""
    root, rb, irb = root.astype(np.float64), rb.astype(np.float64), irb.astype(np.float64)
    ball, paddle = root[:, 2], rb[:, PADDLE_BODY]
    t = dict(bx=ball[:, 0], by=ball[:, 1], bz=ball[:, 2], vx=ball[:, 7], dxp=np.abs(ball[:, 0] - paddle[:, 0]),
             yz=np.hypot(ball[:, 1] - paddle[:, 1], ball[:, 2] - paddle[:, 2]), pelvis_h=rb[:, 0, 2], root_x=root[:, 0, 0],
             disp=np.linalg.norm(rb[:, BAL_IDS, :3] - irb[:, BAL_IDS, :3], axis=-1).mean(axis=1))
    for name, bit in STICKY_BITS.items():
        t[name] = (flags0 & bit) != 0
    return t


def classify(flags0, root, rb, irb, pvx):
    """-> {cell: bool [N]} of one env-step.  flags0: the flag words at the step's start; root / rb / pvx: the oracle's tensors between its
    rigid-body step and its post_physics_step; irb [N or 1, 42, 13]."""
    t = _terms(flags0, root, rb, irb)
    pc, htc, dpc, hd = t["PADDLE_COND"], t["HIT_TABLE_CALC"], t["DIE_PENALTY_CALC"], t["HUMANOID_DIE_CALC"]
    bx, by, bz, vx = t["bx"], t["by"], t["bz"], t["vx"]
    x_close, in_circle = t["dxp"] < 0.2, t["yz"] < 0.15
    first_close = x_close & ~pc
    hit_paddle = (pvx < 0) & (vx > 1.5)
    z_in = (bz >= 0.82) & (bz <= 0.83) & (vx > 0)
    in_range = (bx >= 1.9) & (bx <= 3.1) & (by >= -0.6) & (by <= 0.6)
    over_net = (bx > 1.72) & (bx < 1.78) & (vx > 0)
    height = {"suitable": (bz > 0.96) & (bz < 1.25), "too_high": bz >= 1.25, "too_low": bz <= 0.96}
    below = bz < 0.78
    c = {"first_close/in_circle/hum_die_off": first_close & in_circle & ~hd, "first_close/in_circle/hum_die_on": first_close & in_circle & hd,
         "first_close/miss/hum_die_off": first_close & ~in_circle & ~hd, "first_close/miss/hum_die_on": first_close & ~in_circle & hd,
         "x_close/paddle_cond_set": x_close & pc,
         "hit_paddle/paid": hit_paddle & ~pc & ~hd, "hit_paddle/gated_paddle_cond": hit_paddle & pc, "hit_paddle/gated_hum_die": hit_paddle & ~pc & hd,
         "below/paid": below & ~dpc & ~hd, "below/gated": below & (dpc | hd),
         "has_fallen/true": t["disp"] > 0.32, "has_fallen/false": t["disp"] <= 0.32,
         "pelvis_low/true": t["pelvis_h"] < 0.97, "pelvis_low/false": t["pelvis_h"] >= 0.97}
    for r, m in (("in_range", in_range), ("out_of_range", ~in_range)):
        c[f"z_in/{r}/paid"], c[f"z_in/{r}/gated_hit_table_calc"], c[f"z_in/{r}/gated_hum_die"] = z_in & m & ~htc & ~hd, z_in & m & htc, z_in & m & ~htc & hd
    for h, m in height.items():
        c[f"over_net/{h}/hum_die_off"], c[f"over_net/{h}/hum_die_on"] = over_net & m & ~hd, over_net & m & hd
    on = (bx > t["root_x"]) & (vx < 0)
    c["time_penalty/on"], c["time_penalty/off"] = on, ~on
    assert sorted(c) == sorted(CELLS)
    return c


def near_threshold(flags0, root, rb, irb, pos_tol, rb_tol, vel_tol):
    """The threshold probe: env-steps whose ORACLE post-simulate value lies within the comparison tolerance of a branch threshold, where an
    fp32 kernel inside its tolerance may take the other branch.  pos_tol / rb_tol / vel_tol: the tolerances of the ball's position, a
    body's position and the ball's velocity (TOL["root_pos"], TOL["rb_pos"], TOL["root_vel"] of tests/test_ta_physics.py).  -> bool [N]"""
    t = _terms(flags0, root, rb, irb)
    near = lambda v, thresholds, tol: np.any([np.abs(v - x) <= tol for x in thresholds], axis=0)
    bad = near(t["dxp"], [0.2], pos_tol + rb_tol) | near(t["yz"], [0.15], np.sqrt(2.0) * (pos_tol + rb_tol))
    bad |= near(t["vx"], [1.5, 0.0], vel_tol)
    bad |= near(t["bz"], [0.82, 0.83, 0.96, 1.25, 0.78], pos_tol) | near(t["bx"], [1.9, 3.1, 1.72, 1.78], pos_tol) | near(t["by"], [-0.6, 0.6], pos_tol)
    bad |= near(t["bx"] - t["root_x"], [0.0], 2 * pos_tol)
    bad |= near(t["pelvis_h"], [0.97], rb_tol) | near(t["disp"], [0.32], rb_tol)
    return bad


@functools.lru_cache(maxsize=None)
def oracle_run(n, seed, resets, per_env_irb=False):
    """The reference trajectory of `scenarios(n, seed, resets)`: STEPS steps of the oracle's rigid-body step + post_physics_step.
    -> (params, irb, steps); a step is a dict of the state at its start (root0, dof0, flags0, episode0, progress0, act), the oracle's
    tensors between the two halves (after_sim = root, dof, rb, frc, pvx), its outputs (main = root, dof, rb, frc, obs, rew, reset, progress,
    episode, flags), `switch` (ball_switch_probe), `near` (near_threshold) and `cells` (classify).  Nothing in it is to be written to."""
    import test_ta_physics as tp
    from oracle import binding
    binding.build()
    cfg, m, p = scene.build_ta_scene(n), scene.build_ta_model(), scene.build_ta_params(n, seed=ENV_SEED)
    root, dof, flags, progress, act = scenarios(n, seed, resets)
    stand = np.zeros((1, 3, 13), np.float32)
    for a in range(3):
        stand[0, a, :7] = np.array(list(p.init_root[a]))
    irb = binding.ta_forward_kinematics(m, stand, np.zeros((1, 27, 2), np.float32))       # TA:1152 initial_body_states
    p.initial_rb_shared = 0 if per_env_irb else 1
    if per_env_irb:
        irb = np.ascontiguousarray(np.broadcast_to(irb, (n, 42, 13)))
    episode = np.zeros(n, np.uint32)
    steps = []
    for t in range(STEPS):
        s = dict(root0=root.copy(), dof0=dof.copy(), flags0=flags.copy(), episode0=episode.copy(), progress0=progress.copy(), act=act)
        rb, frc, pvx = binding.ta_simulate(cfg, m, act, root, dof, threads=8)
        s["switch"] = tp.ball_switch_probe(binding, cfg, m, act, s["root0"], s["dof0"], root, seed=300 + t)
        s["near"] = near_threshold(s["flags0"], root, rb, irb, tp.TOL["root_pos"], tp.TOL["rb_pos"], tp.TOL["root_vel"])
        s["cells"] = classify(s["flags0"], root, rb, irb, pvx)
        s["after_sim"] = (root.copy(), dof.copy(), rb, frc, pvx)
        obs, rew, reset = binding.ta_post_physics_step(p, rb, irb, root, dof, frc, pvx, None, flags, episode, progress)
        s["main"] = (root.copy(), dof.copy(), rb, frc, obs, rew, reset, progress.copy(), episode.copy(), flags.copy())
        steps.append(s)
    return p, irb, steps


def cell_counts(steps, keep=None, only_resets=False):
    """-> {cell: env-steps in it}, over the envs that neither probe set aside (keep: per step, instead) and, with only_resets, that reset in
    that step."""
    counts = dict.fromkeys(CELLS, 0)
    for i, s in enumerate(steps):
        k = ~(s["switch"] | s["near"]) if keep is None else keep[i]
        if only_resets:
            k = k & (s["main"][6] != 0)
        for name, mask in s["cells"].items():
            counts[name] += int((mask & k).sum())
    return counts
