"""Scripted states that put the 7-dof (TT / TN / T3) and the 4-actor (T4) step on every branch of the reward and reset decision
(compute_reward / compute_reward_side2, csrc/ppenv_device.h, with the sticky flag word they read and modify), and the oracle-only
book-keeping of the tests that use them (tests/test_reward_branches_host.py / _gpu.py).

The random-action rollouts bring the ball to these branches a handful of env-steps in half a million, and some never.  `scenarios`
starts every env from the variant's created state, holds the arm(s) at a drawn pose (the actions whose PD target it is) and AIMS the ball
through free air (ball_contact_scenarios.launch) so that at the END of step (env % 7) % 3 of STEPS its position and vx lie on the wanted
side of each threshold, at least MARGIN away from it; every threshold also has a slice of balls MARGIN .. 2 MARGIN on either side of it (the edge/ cases and
cells: a threshold moved by EDGE_SHIFT = 0.01 changes what a whole slice is paid).  The case of env e is CASES[variant][e % len(CASES[variant])] (the lengths share no
factor with 7 or 2), on T4 mirrored about the table's centre for humanoid 2 in the odd envs.  The sticky bits a case does not fix are drawn with probability
1/2, per side.  The one branch that no free flight reaches, a ball that TURNS within a step (pre_vx < 0 < vx), is flown into the net's face:
the slab is static and needs no arm, the rebound's vx is restitution x the approach.  A ball placed with vx = 0 (vy = 0) keeps its x (y)
bit for bit through a free step, in fp32 as in fp64 (x + 0 hb): those cases sit EXACTLY on a threshold.  In the reset pass the envs with
env % 7 = 0 / 1 / 2 are 2 / 3 / 4 steps short of max_episode_length, so that they time out in the step their case is aimed at, and those with
env % 7 = 3 end the run at max_episode_length - 2 after the increment: next to the time-out and not in it.

Everything here is decided from the ORACLE and the config, never from a kernel's output.  `oracle_run` steps, from the main oracle's state
at the start of each step, two more oracles: `watch`, whose Config never times out (a reset hides the ball the reward saw), and `parked`,
the same with the ball parked far away (it never resets: its bodies are the main run's pre-reset bodies, for the ball does not move the arm).
`terms` reads the ball the reward saw off `watch` where it did not reset, and where it died off the fp64 free flight of the pre-step state
(ball_contact_scenarios.first_contact) provided that flight met no body; an env-step that died after a contact is in the death cells alone.
`classify` decides the cells from those, the pre-step flags and pre-step vx.  `near_threshold` sets aside the env-steps whose ball coordinate
or vx lies within the comparison tolerance of a threshold its variant compares it with (an fp32 kernel inside its tolerance may take the
other branch; the exactly placed ones excepted); together with SensitivityProbe's they go through check_excluded.

The thresholds below restate the specification's literals; tests/test_reward_branches_host.py measures each of them, and whether it is
strict, off the oracle's tensor-API entry points (ppo_post_physics_step, ppo_t4_rewards) at the fp32 neighbours of the value."""
import functools
import types

import numpy as np

import ball_contact_scenarios as sc
from helpers import RTOL, SCALES, SensitivityProbe, obs_atol, reward_atol
from isaacgym_amd import scene

STEPS = 3
FLOOR = 8                    # kept env-steps every cell must reach, per variant and pass
ENV_SEED = 11
EXCLUDED_BOUND = 0.02
REACHED = 100.0              # x the reward tolerance: the size of a cell's discrete term
MARGIN = 0.004               # m: how far from a threshold the scripted targets are drawn (the comparison tolerance is below 4e-4 m)
VARIANTS = ("TT", "TN", "T3", "T4")
RC, CC, NB, MC = scene.FLAG_REWARD_CALC, scene.FLAG_COND_CALC, scene.FLAG_NO_BOUNCE, scene.FLAG_MISSED_CALC
f32 = np.float32

# ---- the specification's thresholds (side 1 / side 2 of the table; measured off the oracle by test_thresholds_are_the_oracles)
X_HALF = (f32(2.44), f32(1.06))          # the table's far half begins
X_END = (f32(3.1), f32(0.4))             # beyond the table's end (>= / <=)
BACK = f32(0.05)                         # missed: behind the humanoid's root by more than this
Z_BOUNCE, Y_BOUNCE = f32(0.83), f32(0.6)
NET_X, NET_Y, NET_Z, NET_REWARD = (f32(1.7), f32(1.8)), f32(0.4), (f32(0.98), f32(1.14)), 400.0
Z_DIE = f32(0.1)
TN_HIT_VX, TN_PADDLE_BACK, TN_FLOOR_REWARD = f32(1.0), f32(0.1), -800.0
T3_PADDLE_BACK = f32(1e-3)
# TN's pos_reward = exp(-20 dist^2) <= 1 = 4 x its reward tolerance (alpha = 1000 sets it): it cannot be REACHED x the tolerance.  Its gate's cells
# count where the term is at least TN_POS_REACHED x the tolerance; the comparison's own bound there is 1 + RTOL |reward| / tolerance <= 1.4 x.
TN_POS_REACHED = 2.0

# Cells that cannot be reached, each asserted where it is stated:
UNREACHABLE = {
    "T4: exactly one side's reset fires":
        "both sides apply the same rule to the same progress and the same ball height (T4:1270-1276, 1431-1437): reset1 == reset2 on every env-step; "
        "test_t4_sides_reset_together asserts it on the oracle's two reward functions over the run's own inputs",
    "T3: two physical turns in one run":
        "a turn needs a body on either side of the ball within STEPS steps, and T3's scene has the net alone in the ball's way; the missing latch is "
        "pinned by vel_reward/paid_cond_calc_set: a turn with COND_CALC set in the flag word, which TT would not pay",
    "a moving ball exactly ON X_END or X_HALF":
        "a moving ball's x is rounded differently in fp32 and fp64, so it cannot be placed; beyond/exactly_at places Bx = X_END with vx = 0, which the flag's >= sees, but the "
        "penalty at X_END and `early` / `inx` at X_HALF also ask for vx > 0 (side 2: < 0): whether THEIR comparisons are strict shows on no reachable env-step; "
        "test_named_exceptions_stay_unreachable asserts that none exists (as it does for T3's two turns)",
}

_TT = (["vel_reward/paid", "vel_reward/gated_cond_calc", "cond/false_pre_vx", "cond/false_vx", "missed/true", "missed/false", "missed/exactly_at",
        "early/paid", "early/gated_reward_calc", "good/paid", "good/gated_reward_calc", "good/refused_no_bounce_clear",
        "inx/false_near", "inx/false_far", "bounce/false_bz", "bounce/false_vx", "bounce/false_by_high", "bounce/false_by_low", "bounce/false_by_exactly_at",
        "beyond/paid", "beyond/gated_reward_calc", "beyond/vx_not_positive_sets_flag", "beyond/exactly_at",
        "net/in"] + [f"net/out_{k}" for k in ("x_low", "x_high", "vx", "y_high", "y_low", "z_low", "z_high")] +
       ["dies/true", "dies/false"])
# Every threshold also has a slice of balls MARGIN .. 2 MARGIN on either side of it, with the rest of its expression live (a shift of the threshold by
# EDGE_SHIFT = 0.01 > 2 MARGIN changes what every one of them is paid): cells edge/<threshold>/just_below and /just_above
EDGE_SHIFT = 0.01
_TT_EDGES = ["x_half", "x_end", "x_end_bouncing", "back", "z_bounce", "y_bounce_high", "y_bounce_low", "net_x_low", "net_x_high", "net_vx", "net_y_high", "net_y_low", "net_z_low", "net_z_high", "z_die"]
_both = lambda names, pre="edge/": [f"{pre}{k}/{s}" for k in names for s in ("just_below", "just_above")]
_TT = _TT + _both(_TT_EDGES)
_TIME = ["timeout/alone", "timeout/with_paying_branch", "timeout/one_step_short"]
_T3 = ["vel_reward/paid", "vel_reward/paid_cond_calc_set", "vel_reward/none", "missed/true", "missed/false", "dies_low/true", "dies_low/false"] + _both(["paddle_back", "z_die"])
_TN = (["hit_paddle/vx_at_most_1", "hit_paddle/vx_above_1", "missed/humanoid_alone", "missed/paddle_alone", "missed/both", "missed/false",
        "penalty/paid", "penalty/gated_missed_calc", "pos_reward/paid", "pos_reward/closed_cond_calc", "pos_reward/reopened_behind",
        "vel_reward/paid", "vel_reward/gated_cond_calc", "floor/on", "floor/off"] + _both(["back", "paddle_back", "z_die", "pos_back"]) + _both(["vx_1"], "hit_paddle/edge_"))
_T4_DIFFER = [f"differ/{b}/{s}" for b in ("cond_calc", "reward_calc", "no_bounce") for s in ("side1", "side2")]
CELLS = {"TT": _TT, "TN": _TN, "T3": _T3, "T4": _TT + [f"h2/{c}" for c in _TT] + _T4_DIFFER}
RESET_CELLS = {v: CELLS[v] + _TIME for v in VARIANTS}
# cells that need not share an env-step with a time-out in the reset pass (a penalty is gated in the steps AFTER the one the case is aimed at)
NOT_WITH_TIMEOUT = ("penalty/gated_missed_calc",)


def cells_of(variant, resets):
    return (RESET_CELLS if resets else CELLS)[variant]


# ------------------------------------------------------------------------------------------------------------------ the cases
# A flight case: name -> (x, y, z, vx) ranges of the ball at the END of its step, in side 1's frame (None: the defaults below), and the bits it fixes.
_OVER = (0.785, 0.826)                  # over the table top (its face + the ball's radius = 0.78) and below Z_BOUNCE
_FAR_X, _IN_Y, _UP = (2.46, 3.08), (-0.58, 0.58), (1.0, 6.0)
_NETX, _NETY, _NETZ = (1.706, 1.794), (-0.39, 0.39), (0.986, 1.134)


def _flight(x, y, z, vx, **bits):
    return dict(kind="flight", x=x, y=y, z=z, vx=vx, bits=bits)


def _edge(axis, thr, x, y, z, vx, **bits):
    """A flight whose coordinate `axis` (0, 1, 2: x, y, z; "vx") is drawn MARGIN .. 2 MARGIN below (even rounds of the case cycle) or above (odd rounds)
    the threshold `thr` (a number; "back": the root's x - BACK) instead of from its range."""
    return dict(kind="flight", x=x, y=y, z=z, vx=vx, bits=bits, edge=(axis, thr))


_ANY = (0.0, 0.0)                       # the range of the coordinate an edge case overrides


_TT_CASES = [
    ("good/paid", _flight(_FAR_X, _IN_Y, _OVER, _UP, NB=1, RC=0)),
    ("good/gated", _flight(_FAR_X, _IN_Y, _OVER, _UP, NB=1, RC=1)),
    ("good/refused", _flight(_FAR_X, _IN_Y, _OVER, _UP, NB=0, RC=0)),
    ("early/paid_over", _flight((1.85, 2.42), _IN_Y, _OVER, _UP, RC=0)),
    ("early/paid_under", _flight((1.0, 2.42), _IN_Y, (0.3, 0.64), _UP, RC=0)),
    ("early/gated", _flight((1.0, 2.42), _IN_Y, (0.3, 0.64), _UP, RC=1)),
    ("bounce/bz", _flight(_FAR_X, _IN_Y, (0.835, 0.95), _UP, NB=1, RC=0)),
    ("bounce/vx", _flight(_FAR_X, _IN_Y, _OVER, (-6.0, -1.0), NB=1, RC=0)),
    ("bounce/by_high", _flight(_FAR_X, (0.605, 0.74), _OVER, _UP, NB=1, RC=0)),
    ("bounce/by_low", _flight(_FAR_X, (-0.74, -0.605), _OVER, _UP, NB=1, RC=0)),
    ("bounce/by_exact", dict(kind="exact_y", x=_FAR_X, z=_OVER, vx=_UP, bits=dict(NB=1, RC=0))),
    ("inx/far", _flight((3.16, 3.4), _IN_Y, (0.3, 0.64), _UP, RC=0)),
    ("beyond/paid", _flight((3.105, 3.4), (-0.7, 0.7), (0.9, 1.4), _UP, RC=0)),
    ("beyond/gated", _flight((3.105, 3.4), (-0.7, 0.7), (0.9, 1.4), _UP, RC=1)),
    ("beyond/vx_negative", _flight((3.105, 3.4), (-0.7, 0.7), (0.9, 1.4), (-6.0, -1.0), RC=0)),
    ("beyond/exact", dict(kind="exact_x", which="end", y=(-0.7, 0.7), z=(0.9, 1.4), bits=dict(RC=0))),
    ("net/in", _flight(_NETX, _NETY, _NETZ, _UP)),
    ("net/x_low", _flight((1.62, 1.694), _NETY, _NETZ, _UP)),
    ("net/x_high", _flight((1.806, 1.88), _NETY, _NETZ, _UP)),
    ("net/vx", _flight(_NETX, _NETY, _NETZ, (-6.0, -1.0))),
    ("net/y_high", _flight(_NETX, (0.406, 0.6), _NETZ, _UP)),
    ("net/y_low", _flight(_NETX, (-0.6, -0.406), _NETZ, _UP)),
    ("net/z_low", _flight(_NETX, _NETY, (0.945, 0.974), _UP)),
    ("net/z_high", _flight(_NETX, _NETY, (1.146, 1.3), _UP)),
    ("dies/true", _flight((3.2, 3.45), (-0.7, 0.7), (0.035, 0.094), _UP)),
    ("dies/false", _flight((3.2, 3.45), (-0.7, 0.7), (0.106, 0.2), _UP)),
    ("missed/true", _flight((-0.5, -0.07), (0.5, 0.85), (0.9, 1.5), (-6.0, -1.0))),
    ("missed/exact", dict(kind="exact_x", which="back", y=(0.5, 0.85), z=(0.9, 1.5), bits={})),
    ("turn/paid", dict(kind="turn", speed=(2.0, 6.0), bits=dict(CC=0))),
    ("turn/gated", dict(kind="turn", speed=(2.0, 6.0), bits=dict(CC=1))),
    ("turn/paid_again", dict(kind="turn", speed=(2.0, 6.0), bits=dict(CC=0))),
    ("edge/x_half", _edge(0, float(X_HALF[0]), _ANY, _IN_Y, _OVER, _UP, NB=1, RC=0)),
    ("edge/x_end", _edge(0, float(X_END[0]), _ANY, (-0.7, 0.7), (0.9, 1.4), _UP, RC=0)),
    ("edge/x_end_bouncing", _edge(0, float(X_END[0]), _ANY, _IN_Y, _OVER, _UP, NB=1, RC=0)),      # `inx`'s far bound: hit_table_reward inside, the penalty beyond
    ("edge/x_half_again", _edge(0, float(X_HALF[0]), _ANY, _IN_Y, _OVER, _UP, NB=1, RC=0)),
    ("edge/back", _edge(0, "back", _ANY, (0.5, 0.85), (0.9, 1.5), (-6.0, -1.0))),
    ("edge/z_bounce", _edge(2, float(Z_BOUNCE), _FAR_X, _IN_Y, _ANY, _UP, NB=1, RC=0)),
    ("edge/y_bounce_high", _edge(1, float(Y_BOUNCE), _FAR_X, _ANY, _OVER, _UP, NB=1, RC=0)),
    ("edge/y_bounce_low", _edge(1, -float(Y_BOUNCE), _FAR_X, _ANY, _OVER, _UP, NB=1, RC=0)),
    ("edge/net_x_low", _edge(0, float(NET_X[0]), _ANY, _NETY, _NETZ, _UP)),
    ("edge/net_x_high", _edge(0, float(NET_X[1]), _ANY, _NETY, _NETZ, _UP)),
    ("edge/net_vx", _edge("vx", 0.0, _NETX, _NETY, _NETZ, _ANY)),
    ("edge/net_y_high", _edge(1, float(NET_Y), _NETX, _ANY, _NETZ, _UP)),
    ("edge/net_y_low", _edge(1, -float(NET_Y), _NETX, _ANY, _NETZ, _UP)),
    ("edge/net_z_low", _edge(2, float(NET_Z[0]), _NETX, _NETY, _ANY, _UP)),
    ("edge/net_z_high", _edge(2, float(NET_Z[1]), _NETX, _NETY, _ANY, _UP)),
    ("edge/z_die", _edge(2, float(Z_DIE), (3.2, 3.45), (-0.7, 0.7), _ANY, _UP)),
]
_T3_CASES = [
    ("turn/paid", dict(kind="turn", speed=(2.0, 6.0), bits=dict(CC=0))),
    ("turn/latched", dict(kind="turn", speed=(2.0, 6.0), bits=dict(CC=1))),
    ("missed/true", dict(kind="behind_paddle", back=(0.01, 0.3), bits={})),
    ("missed/false", dict(kind="behind_paddle", back=(-0.3, -0.01), bits={})),
    ("dies/true", _flight((3.2, 3.45), (-0.7, 0.7), (0.035, 0.094), _UP)),
    ("dies/false", _flight((3.2, 3.45), (-0.7, 0.7), (0.106, 0.2), _UP)),
    ("flight", _flight((1.0, 3.0), (-0.7, 0.7), (0.9, 1.4), (-6.0, 6.0))),
    ("turn/paid_again", dict(kind="turn", speed=(2.0, 6.0), bits=dict(CC=0))),
    ("missed/true_again", dict(kind="behind_paddle", back=(0.01, 0.3), bits={})),
    ("edge/paddle_back", dict(kind="behind_paddle", back=_ANY, bits={}, edge=(0, "t3_paddle"))),
    ("edge/z_die", _edge(2, float(Z_DIE), (3.2, 3.45), (-0.7, 0.7), _ANY, _UP)),
]
_TN_CASES = [
    ("turn/slow", dict(kind="turn", speed=(0.6, 1.8), bits=dict(CC=0))),
    ("turn/paid", dict(kind="turn", speed=(2.4, 6.0), bits=dict(CC=0))),
    ("turn/gated", dict(kind="turn", speed=(2.4, 6.0), bits=dict(CC=1))),
    ("missed/both", dict(kind="tn_missed", which="both", bits=dict(MC=0))),
    ("missed/paddle_alone", dict(kind="tn_missed", which="paddle", bits=dict(MC=0))),
    ("missed/humanoid_alone", dict(kind="tn_missed", which="humanoid", bits=dict(MC=0))),
    ("missed/gated", dict(kind="tn_missed", which="both", bits=dict(MC=1))),
    ("pos/paid", dict(kind="tn_pos", behind=False, bits=dict(CC=0))),
    ("pos/closed", dict(kind="tn_pos", behind=False, bits=dict(CC=1))),
    ("pos/reopened", dict(kind="tn_pos", behind=True, bits=dict(CC=1))),
    ("floor/on", _flight((3.2, 3.45), (-0.7, 0.7), (0.035, 0.094), _UP)),
    ("floor/off", _flight((3.2, 3.45), (-0.7, 0.7), (0.106, 0.2), _UP)),
    ("missed/humanoid_alone_again", dict(kind="tn_missed", which="humanoid", bits=dict(MC=0))),
    ("edge/vx_1", dict(kind="turn", speed=_ANY, bits=dict(CC=0), edge=("speed", float(TN_HIT_VX)))),
    ("edge/back", dict(kind="tn_missed", which="humanoid", bits=dict(MC=0), edge=(0, "back"))),
    ("edge/paddle_back", dict(kind="tn_missed", which="paddle", bits=dict(MC=0), edge=(0, "tn_paddle"))),
    ("edge/z_die", _edge(2, float(Z_DIE), (3.2, 3.45), (-0.7, 0.7), _ANY, _UP)),
    ("edge/pos_back", dict(kind="tn_pos", behind=True, pose="any", bits=dict(CC=1, MC=1), edge=(0, "back"))),
    ("edge/pos_back_again", dict(kind="tn_pos", behind=True, pose="any", bits=dict(CC=1, MC=1), edge=(0, "back"))),
]
CASES = {"TT": _TT_CASES, "T4": _TT_CASES, "T3": _T3_CASES, "TN": _TN_CASES}
for _v, _c in CASES.items():
    assert len(_c) % 7 and len(_c) % 2, (_v, len(_c))        # the case, the step rule (env % 7) and T4's side (env % 2) cycle independently


def case_of(variant, n):
    """-> (case index [n], side [n]: 0, or on T4 env % 2)."""
    env = np.arange(n)
    return env % len(CASES[variant]), (env % 2 if variant == "T4" else 0 * env)


def mirror_x(cfg, x):
    return 2.0 * float(cfg.table.center[0]) - x


def scenarios(variant, n, seed, resets=False):
    """-> (state blob of the oracle at the start, actions [n A, 7] held over the STEPS steps, meta: case / side / when / exact [n])."""
    from oracle import binding
    binding.build()
    cfg = scene.build_config(variant, num_envs=n, seed=ENV_SEED)
    o = binding.OracleEnv(cfg, threads=8)
    A = cfg.num_humanoids
    per, hb = sc._micro(cfg)
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    env = np.arange(n)
    case, side = case_of(variant, n)
    when = (env % 7) % 3
    cases = CASES[variant]
    r, off = float(cfg.ball_radius), float(cfg.contact_offset)
    g = float(cfg.gravity_z)
    A = cfg.num_humanoids
    hx = float(cfg.humanoid_root_pos[0])
    # the heights the cases' ranges take for granted, against the scene: over the table's face and the net's top edge by more than the ball's radius, the
    # turn's band on the net's face and over the table, the lowest target over the ground
    table_top, net_top = (float(b.center[2]) + float(b.half[2]) for b in (cfg.table, cfg.net))
    assert table_top + r + off < _OVER[0] - 0.004 and net_top + r + off < 0.945 - 0.004 and table_top + r + off < 0.80 and 0.89 < net_top
    assert float(cfg.table.center[2]) - float(cfg.table.half[2]) - r - off > 0.64 + 0.05 and float(cfg.ground_z) + r + off < 0.035 - 0.004
    side_sign = np.where((env // (len(cases) * A)) % 2 == 0, -1.0, 1.0)       # an edge case's side of its threshold: by rounds of the (case, side) cycle
    beside = lambda: side_sign * u(MARGIN, 2 * MARGIN)

    # ---- the arms: a pose strictly inside the limits, at rest, held by the actions (ball_contact_scenarios); TN's "humanoid alone" needs the blade
    #      behind the root: the arm swung back
    lo, hi = (np.array([getattr(cfg.joint[j], k) for j in range(7)], np.float64) for k in ("lower", "upper"))
    q = rng.uniform(-0.5, 0.5, (A, 7, n))
    if variant == "TN":
        back = np.array([c[1].get("which") == "humanoid" for c in cases])[case]
        q[0, 0, back], q[0, 3, back] = u(1.8, 2.4)[back], u(0.3, 1.0)[back]
        # the gate that reopens pos_reward behind the root: the ball beside the root's line AND within 0.12 m of the blade's (y, z) is in free air only for
        # some poses: drawn over the whole range, the env-steps whose flight meets a body are not counted
        wide = np.array([c[1].get("pose") == "any" for c in cases])[case]
        q[0][:, wide] = rng.uniform(lo[:, None], hi[:, None], (7, n))[:, wide]
    q = np.clip(q, (lo + 0.01)[None, :, None], (hi - 0.01)[None, :, None])
    actions = np.clip((q - 0.5 * (hi + lo)[None, :, None]) / (0.5 * (hi - lo))[None, :, None], -1, 1)
    actions = np.ascontiguousarray(actions.transpose(2, 0, 1).reshape(n * A, 7), np.float32)
    o.dof_pos[:], o.dof_vel[:] = q.reshape(A * 7, n), 0.0
    o.ball[0:3] = np.array([[10.0], [10.0], [5.0]])
    o.ball[7:13] = 0.0
    start = o.get_state()
    paddles = []                                               # first pass, the ball parked: where blade 1 is at the END of each step
    for t in range(STEPS):
        o.step(actions)
        assert not o.reset_buf.any()
        paddles.append(o.refresh_rigid_body_states()[:, 39, :3].astype(np.float64))
    paddle = np.stack(paddles)[when, env]

    # ---- the ball at the end of step `when` (flight cases) or at a contact test inside it (turn cases)
    P, V = np.zeros((n, 3)), np.zeros((n, 3))
    M = (when + 1) * per                                       # launch's micro-step count: the position after step `when`
    exact = np.zeros(n, bool)
    bits = rng.integers(0, 2, (A, n, 4)).astype(bool)          # RC, CC, NB, MC per side
    if variant == "TN":
        bits[:, :, 2] = True                                   # TN never touches NO_BOUNCE: it stays as created
    else:
        bits[:, :, 3] = False
    col = dict(RC=0, CC=1, NB=2, MC=3)
    for ci, (name, c) in enumerate(cases):
        m = case == ci
        for b, val in c["bits"].items():
            for a in range(A):
                bits[a, m & (side == a), col[b]] = bool(val)
        k = c["kind"]
        if k == "flight":
            P[m] = np.stack([u(*c["x"]), u(*c["y"]), u(*c["z"])], 1)[m]
            V[m] = np.stack([u(*c["vx"]), u(-0.5, 0.5), u(-1.5, 1.5)], 1)[m]
        elif k == "exact_y":                                   # By = +-Y_BOUNCE bit for bit: vy = 0
            P[m] = np.stack([u(*c["x"]), rng.choice([-1.0, 1.0], n) * float(Y_BOUNCE), u(*c["z"])], 1)[m]
            V[m] = np.stack([u(*c["vx"]), 0 * env, u(-1.5, 1.5)], 1)[m]
            exact |= m
        elif k == "exact_x":                                   # Bx = the threshold bit for bit: vx = 0 (side 2's value is set after the mirror)
            P[m] = np.stack([np.full(n, float(X_END[0]) if c["which"] == "end" else float(f32(hx) - BACK)), u(*c["y"]), u(*c["z"])], 1)[m]
            V[m] = np.stack([0.0 * env, u(-0.5, 0.5), u(-1.5, 1.5)], 1)[m]
            exact |= m
        elif k == "turn":                                      # into the net's far face (side 2: its near face), from over the table and below the net's top edge
            c0, h0 = np.array(list(cfg.net.center), np.float64), np.array(list(cfg.net.half), np.float64)
            sp = u(*c["speed"])
            if "edge" in c:                                    # the rebound's vx = restitution x the approach, beside the threshold
                sp = (c["edge"][1] + beside()) / float(cfg.net.restitution)
            s = off - u(0.15, 0.85) * sp * hb                  # separation at the activating micro-step: outside the zone one micro-step earlier
            P[m] = np.stack([c0[0] + h0[0] + r + s, u(-0.7, 0.7), u(0.80, 0.89)], 1)[m]
            V[m] = np.stack([-sp, u(-0.5, 0.5), u(-0.3, 0.3)], 1)[m]
            M = np.where(m, when * per + rng.integers(0, per - 1, n), M)
        elif k == "behind_paddle":                             # T3: beside the blade (0.25 - 0.5 m from its centre in y, z), before or behind it in x
            ang = u(0.2, 2.9)
            rad = u(0.25, 0.5)
            P[m] = (paddle + np.stack([-u(*c["back"]), rad * np.cos(ang), rad * np.sin(ang)], 1))[m]
            V[m] = np.stack([u(-6.0, -1.0), u(-0.3, 0.3), u(-0.5, 0.5)], 1)[m]
        elif k == "tn_missed":
            w = c["which"]
            # both: behind the root and the blade; paddle alone: between the root's line and the blade's; humanoid alone: behind the root, the blade further back
            if w == "both":
                x = np.minimum(hx - float(BACK), paddle[:, 0] - float(TN_PADDLE_BACK)) - u(0.02, 0.3)
            elif w == "paddle":
                lo_x, hi_x = hx - float(BACK) + MARGIN, paddle[:, 0] - float(TN_PADDLE_BACK) - MARGIN
                x = lo_x + u(0.0, 1.0) * np.maximum(hi_x - lo_x, 0.0)
            else:
                lo_x, hi_x = paddle[:, 0] - float(TN_PADDLE_BACK) + MARGIN, hx - float(BACK) - MARGIN
                x = lo_x + u(0.0, 1.0) * np.maximum(hi_x - lo_x, 0.0)
            P[m] = np.stack([x, u(0.55, 0.9), u(0.9, 1.5)], 1)[m]
            V[m] = np.stack([u(-4.0, -1.0), u(-0.3, 0.3), u(-0.5, 0.5)], 1)[m]
        elif k == "tn_pos":                                    # within 0.12 m of the blade's (y, z): over the table, or (reopened) behind the root
            ang, rad = u(0, 2 * np.pi), u(0.0, 0.12)
            x = u(hx - 0.6, hx - 0.3) if c["behind"] else u(1.0, 1.6)
            P[m] = np.stack([x, paddle[:, 1] + rad * np.cos(ang), np.maximum(paddle[:, 2] + rad * np.sin(ang), 0.9)], 1)[m]
            V[m] = np.stack([u(-4.0, -1.0), u(-0.2, 0.2), u(-0.3, 0.3)], 1)[m]
        if "edge" in c and k != "turn":
            axis, thr = c["edge"]
            thr = {"back": hx - float(BACK), "tn_paddle": paddle[:, 0] - float(TN_PADDLE_BACK), "t3_paddle": paddle[:, 0] - float(T3_PADDLE_BACK)}.get(thr, thr)
            if axis == "vx":
                V[m, 0] = (thr + beside())[m]
            else:
                P[m, axis] = (thr + beside())[m]
    # a target in the band between the table's face and Z_BOUNCE is met falling, fast enough to have been above Z_BOUNCE one step earlier: the steps
    # before the aimed one do not bounce, and leave the flag word as the case set it
    band = (P[:, 2] > table_top) & (P[:, 2] < float(Z_BOUNCE) + 2.5 * MARGIN) & (V[:, 2] != 0)
    V[:, 2] = np.where(band, -np.maximum(0.3, (float(Z_BOUNCE) + 0.006 - P[:, 2]) / float(cfg.dt) * u(1.05, 1.5)), V[:, 2])
    second = side == 1
    P[second, 0], P[second, 1] = mirror_x(cfg, P[second, 0]), -P[second, 1]
    V[second, 0], V[second, 1] = -V[second, 0], -V[second, 1]
    if variant == "T4":
        for ci, (name, c) in enumerate(cases):
            if c["kind"] == "exact_x":
                m = (case == ci) & second
                P[m, 0] = float(X_END[1]) if c["which"] == "end" else float(f32(cfg.humanoid2_root_pos[0]) + BACK)
    V[:, 2] += g * hb                                          # launch's velocity is the one after the NEXT micro-step's kick
    p0, v0 = sc.launch(cfg, P, V, M)
    p0, v0 = p0.astype(np.float32), v0.astype(np.float32)
    ex = exact & np.array([c[1]["kind"] == "exact_x" for c in cases])[case]
    ey = exact & ~ex
    p0[ex, 0], v0[ex, 0] = P[ex, 0].astype(np.float32), 0.0
    p0[ey, 1], v0[ey, 1] = P[ey, 1].astype(np.float32), 0.0
    o.set_state(start)
    o.ball[0:3], o.ball[7:10] = p0.T, v0.T
    o.ball[10:13] = rng.uniform(-30, 30, (3, n))
    flags = (bits * np.array([RC, CC, NB, MC])).sum(axis=2).astype(np.uint32)
    o.flags[...] = flags[0] if A == 1 else flags
    L = int(cfg.max_episode_length)
    progress = rng.integers(0, L - 3 - STEPS, n)               # nobody times out inside the run
    if resets:
        for k in range(STEPS):
            progress[env % 7 == k] = L - 2 - k                 # time out in step k
        progress[env % 7 == 3] = L - 2 - STEPS                 # end the run one step short of it
    o.progress_buf[:] = np.repeat(progress, A)
    blob = o.get_state()
    o.close()
    return blob, actions, dict(case=case, side=side, when=when, exact=exact)


# ------------------------------------------------------------------------------------------------------------------ what the reward saw
def never_times_out(cfg):
    c = sc._copy(cfg)
    c.max_episode_length = 1 << 30
    return c


def terms(cfg, ball0, rb0, watch, parked_rb):
    """The quantities the branches compare, as float32 (what the oracle's reward compares): bx, by, bz, vx at the end of the step before any reset,
    pre_vx, blade positions, and `known` [n]: False where `watch` died after a contact (its pre-reset ball is not on record).  ball0 / rb0: the
    oracle's ball [13, n] and refresh_rigid_body_states() at the step's start; watch: snapshot of the oracle that never times out after the step;
    parked_rb: refresh_rigid_body_states() of the oracle with the ball parked after it."""
    n, A = ball0.shape[1], cfg.num_humanoids
    died = watch.reset_buf.reshape(n, A)[:, 0] != 0
    _, found, _, p_end = sc.first_contact(cfg, ball0, rb0)
    ball = np.where(died[None, :], np.nan, watch.ball[[0, 1, 2, 7]].astype(np.float64))
    free = died & ~found
    ball[0:3, free] = p_end[free].T
    ball[3, free] = ball0[7, free]
    t = dict(zip(("bx", "by", "bz", "vx"), ball.astype(np.float32)))
    t.update(known=~died | free, died=died, free_flight=~found, p_end=p_end, pre_vx=ball0[7].astype(np.float32), vy0=ball0[8].astype(np.float32),
             paddle=[parked_rb[:, scene.NUM_HUMANOID_BODIES * a + 39, :3].astype(np.float32) for a in range(A)])
    return t


def _side(cfg, t, a):
    """The side's frame: sg (+1 / -1), sg x the ball's x / vx / pre_vx, sg x its thresholds (the comparisons of side 2 are side 1's mirrored)."""
    sg = f32(1.0) if a == 0 else f32(-1.0)
    root = f32(cfg.humanoid_root_pos[0]) - BACK if a == 0 else f32(cfg.humanoid2_root_pos[0]) + BACK
    return sg, sg * t["bx"], sg * t["vx"], sg * t["pre_vx"], sg * X_HALF[a], sg * X_END[a], sg * root


def _tt_side(cfg, t, flags0, a):
    """-> (cells of TT's function on side a, events: the booleans the flag word changes on)."""
    sg, x, vx, pvx, half, end, root = _side(cfg, t, a)
    rc, cc, nb = ((flags0 & b) != 0 for b in (RC, CC, NB))
    k = t["known"]
    by, bz = t["by"], t["bz"]
    cond = (pvx < 0) & (vx > 0) & k
    missed = (x < root) & k
    in_y = (by < Y_BOUNCE) & (by > -Y_BOUNCE)
    bounce = (bz < Z_BOUNCE) & (vx > 0) & in_y & k
    early = (x < half) & bounce
    inx = (x > half) & (x < end) & k
    nb_then = nb & ~early                                      # the early branch clears NO_BOUNCE before `good` reads it
    good = inx & bounce & nb_then
    rc_then = rc | early | good
    beyond = (x >= end) & k
    on_table = (x < end) & k                                   # where `bounce` is read by one of the two branches
    exact_y = (np.abs(by) == Y_BOUNCE) & (t["vy0"] == 0)
    net = [t["bx"] > NET_X[0], t["bx"] < NET_X[1], vx > 0, by < NET_Y, by > -NET_Y, bz > NET_Z[0], bz < NET_Z[1]]
    others = lambda i: np.all([c for j, c in enumerate(net) if j != i], axis=0)
    c = {"vel_reward/paid": cond & ~cc, "vel_reward/gated_cond_calc": cond & cc,
         "cond/false_pre_vx": ~(pvx < 0) & (vx > 0) & k, "cond/false_vx": (pvx < 0) & ~(vx > 0) & k,
         "missed/true": missed, "missed/false": ~missed & k & ~(x == root), "missed/exactly_at": (x == root) & k & (t["pre_vx"] == 0),
         "early/paid": early & ~rc, "early/gated_reward_calc": early & rc,
         "good/paid": good & ~rc, "good/gated_reward_calc": good & rc, "good/refused_no_bounce_clear": inx & bounce & ~nb & ~rc,
         "inx/false_near": bounce & (x < half), "inx/false_far": bounce & (x >= end),
         "bounce/false_bz": on_table & ~(bz < Z_BOUNCE) & (vx > 0) & in_y & inx & nb & ~rc, "bounce/false_vx": on_table & (bz < Z_BOUNCE) & ~(vx > 0) & in_y & inx & nb & ~rc,
         "bounce/false_by_high": on_table & (bz < Z_BOUNCE) & (vx > 0) & ~(by < Y_BOUNCE) & inx & nb & ~rc & ~exact_y,
         "bounce/false_by_low": on_table & (bz < Z_BOUNCE) & (vx > 0) & ~(by > -Y_BOUNCE) & inx & nb & ~rc & ~exact_y,
         "bounce/false_by_exactly_at": on_table & (bz < Z_BOUNCE) & (vx > 0) & exact_y & inx & nb & ~rc,
         "beyond/paid": beyond & (vx > 0) & ~rc_then & ~(x == end), "beyond/gated_reward_calc": beyond & (vx > 0) & rc_then,
         "beyond/vx_not_positive_sets_flag": beyond & ~(vx > 0) & ~rc_then & ~(x == end), "beyond/exactly_at": (x == end) & k & (t["pre_vx"] == 0) & ~rc_then,
         "net/in": np.all(net, axis=0) & k,
         "dies/true": t["died"], "dies/false": ~t["died"] & (bz < 0.3) & k}
    for i, name in enumerate(("x_low", "x_high", "vx", "y_high", "y_low", "z_low", "z_high")):
        c[f"net/out_{name}"] = others(i) & ~net[i] & k
    zone = (bz < Z_BOUNCE) & (vx > 0) & inx & nb & ~rc          # where `good` pays: each of its conditions decides alone
    edges = {"x_half": (x, half, bounce & ~rc & nb), "x_end": (x, end, (vx > 0) & ~rc & ~bounce), "x_end_bouncing": (x, end, bounce & (x > half) & nb & ~rc), "back": (x, root, k),
             "z_bounce": (bz, Z_BOUNCE, (vx > 0) & in_y & inx & nb & ~rc), "y_bounce_high": (by, Y_BOUNCE, zone), "y_bounce_low": (by, -Y_BOUNCE, zone),
             "net_x_low": (t["bx"], NET_X[0], others(0)), "net_x_high": (t["bx"], NET_X[1], others(1)), "net_vx": (vx, f32(0.0), others(2)),
             "net_y_high": (by, NET_Y, others(3)), "net_y_low": (by, -NET_Y, others(4)), "net_z_low": (bz, NET_Z[0], others(5)),
             "net_z_high": (bz, NET_Z[1], others(6)), "z_die": (bz, Z_DIE, k)}
    c.update(edge_cells(edges, k))
    for name in c:                                             # every cell but the turn's is aimed through free air, and counted there alone
        if not name.startswith("vel_reward/"):
            c[name] = c[name] & t["free_flight"]
    ev = dict(cond=cond, hit=early | good | (beyond & (vx > 0)), good=inx & bounce & ~early & ~rc,
              pays=(cond & ~cc) | (early & ~rc) | (good & ~rc) | (beyond & (vx > 0) & ~rc_then) | (np.all(net, axis=0) & k) | missed)
    return c, ev


def edge_cells(edges, known, pre="edge/"):
    """{name: (value, threshold, live)} -> the cells name/just_below, name/just_above: the value within 2 MARGIN of the threshold on that side (0.1 mm of
    slack for the rounding of the flight) where the rest of the expression is live."""
    out = {}
    for name, (v, thr, live) in edges.items():
        d = np.nan_to_num(v.astype(np.float64) - np.asarray(thr, np.float64), nan=1e9)
        out[f"{pre}{name}/just_below"] = (d < 0) & (d >= -2 * MARGIN - 1e-4) & live & known
        out[f"{pre}{name}/just_above"] = (d > 0) & (d <= 2 * MARGIN + 1e-4) & live & known
    return out


def classify(cfg, t, flags0, progress_after, resets):
    """-> {cell: bool [n]} of one env-step.  t: terms(); flags0: the flag words at the step's start ([n] or [A, n]); progress_after: the step's
    progress after the increment (its start's + 1); resets: the pass (adds the time-out cells)."""
    variant = {v: k for k, v in scene.VARIANT_IDS.items()}[cfg.variant]
    A, k = cfg.num_humanoids, t["known"]
    flags0 = np.asarray(flags0).reshape(A, -1)
    vx, pvx, bx, bz = t["vx"], t["pre_vx"], t["bx"], t["bz"]
    alpha = abs(float(cfg.alpha_velocity_reward))
    ra = (2 if A == 2 else 1) * reward_atol(cfg)
    big = alpha * np.abs(np.nan_to_num(vx.astype(np.float64))) >= REACHED * ra        # a vel_reward counts where it is REACHED x the tolerance
    if variant in ("TT", "T4"):
        c, ev = _tt_side(cfg, t, flags0[0], 0)
        pays = ev["pays"]
        for name in ("vel_reward/paid", "vel_reward/gated_cond_calc"):
            c[name] = c[name] & big
        if A == 2:
            c2, ev2 = _tt_side(cfg, t, flags0[1], 1)
            for name in ("vel_reward/paid", "vel_reward/gated_cond_calc"):
                c2[name] = c2[name] & big
            c.update({f"h2/{name}": m for name, m in c2.items()})
            pays = pays | ev2["pays"]
            for bit, key, name in ((CC, "cond", "cond_calc"), (RC, "hit", "reward_calc"), (NB, "good", "no_bounce")):
                differ = ((flags0[0] ^ flags0[1]) & bit) != 0
                # the side's outcome turns on the bit: reading the other side's word pays (or gates) what this side's does not
                live = {"cond": lambda e: e["cond"] & big, "hit": lambda e: e["hit"], "good": lambda e: e["good"]}[key]
                c[f"differ/{name}/side1"], c[f"differ/{name}/side2"] = differ & live(ev), differ & live(ev2)
    elif variant == "T3":
        turn = (pvx < 0) & (vx > 0) & k & big
        cc = (flags0[0] & CC) != 0
        missed = (bx < t["paddle"][0][:, 0] - T3_PADDLE_BACK) & k
        low = (bz < Z_DIE) & k
        c = {"vel_reward/paid": turn & ~cc, "vel_reward/paid_cond_calc_set": turn & cc, "vel_reward/none": ~((pvx < 0) & (vx > 0)) & k,
             "missed/true": missed, "missed/false": ~missed & k, "dies_low/true": low & ~missed, "dies_low/false": ~low & (bz < 0.3) & k}
        c.update(edge_cells({"paddle_back": (bx, t["paddle"][0][:, 0] - T3_PADDLE_BACK, k), "z_die": (bz, Z_DIE, ~missed & k)}, k))
        pays = turn | missed
        c = {name: m if name.startswith("vel_reward/pa") else m & t["free_flight"] for name, m in c.items()}
    else:
        cc, mc = ((flags0[0] & b) != 0 for b in (CC, MC))
        root = f32(cfg.humanoid_root_pos[0]) - BACK
        hum, pad = (bx < root) & k, (bx < t["paddle"][0][:, 0] - TN_PADDLE_BACK) & k
        missed = hum | pad
        d2 = (t["paddle"][0][:, 1].astype(np.float64) - t["by"]) ** 2 + (t["paddle"][0][:, 2].astype(np.float64) - bz) ** 2
        pos_big = np.exp(-20.0 * np.nan_to_num(d2, nan=1e9)) >= TN_POS_REACHED * ra
        slow, hit = (pvx < 0) & (vx > 0) & ~(vx > TN_HIT_VX) & k, (pvx < 0) & (vx > TN_HIT_VX) & k & big
        low = (bz < Z_DIE) & k
        c = {"hit_paddle/vx_at_most_1": slow & ~cc, "hit_paddle/vx_above_1": hit,
             "missed/humanoid_alone": hum & ~pad, "missed/paddle_alone": pad & ~hum, "missed/both": hum & pad, "missed/false": ~missed & k,
             "penalty/paid": missed & ~mc, "penalty/gated_missed_calc": missed & mc,
             "pos_reward/paid": ~cc & ~hum & pos_big & k, "pos_reward/closed_cond_calc": cc & ~hum & pos_big & k, "pos_reward/reopened_behind": cc & hum & pos_big,
             "vel_reward/paid": hit & ~cc, "vel_reward/gated_cond_calc": hit & cc, "floor/on": low, "floor/off": ~low & (bz < 0.3) & k}
        c.update(edge_cells({"back": (bx, root, ~pad & ~mc), "paddle_back": (bx, t["paddle"][0][:, 0] - TN_PADDLE_BACK, ~hum & ~mc), "z_die": (bz, Z_DIE, k)}, k))
        c.update(edge_cells({"pos_back": (bx, root, cc & pos_big)}, k))
        c.update(edge_cells({"vx_1": (vx, TN_HIT_VX, (pvx < 0) & ~cc)}, k, "hit_paddle/edge_"))
        pays = (hit & ~cc) | (missed & ~mc) | low
        c = {name: m if name.split("/")[0] in ("hit_paddle", "vel_reward") else m & t["free_flight"] for name, m in c.items()}
    if resets:
        L = int(cfg.max_episode_length)
        out = progress_after >= L - 1
        c["timeout/alone"], c["timeout/with_paying_branch"] = out & ~pays & k, out & pays
        c["timeout/one_step_short"] = (progress_after == L - 2) & ~t["died"]
    return c


def near_threshold(cfg, t):
    """The threshold probe: env-steps whose ball coordinate or vx, as the ORACLE's reward saw it, lies within the comparison tolerance of a threshold
    its variant compares it with.  The tolerances are the comparison's own (RTOL x SCALES + RTOL |threshold|; a threshold relative to the blade adds
    a body position's, obs_atol()[0]), as tests/ta_branch_scenarios.near_threshold takes them.  A coordinate whose velocity component is exactly zero
    before and after the step has not moved by a bit in either precision: it is never near.  -> bool [n]"""
    variant = {v: k for k, v in scene.VARIANT_IDS.items()}[cfg.variant]
    bx, by, bz, vx = (t[k_].astype(np.float64) for k_ in ("bx", "by", "bz", "vx"))
    pos = lambda thr: RTOL * SCALES["ball_pos"] + RTOL * abs(float(thr))
    vel = lambda thr: RTOL * SCALES["ball_vel"] + RTOL * abs(float(thr))
    moving_x, moving_y = ~((t["pre_vx"] == 0) & (t["vx"] == 0)), t["vy0"] != 0
    near = lambda v, thrs, tol: np.any([np.abs(v - float(x)) <= tol(x) for x in thrs], axis=0)
    hx = float(f32(cfg.humanoid_root_pos[0]) - BACK)
    px = t["paddle"][0][:, 0].astype(np.float64)
    body = float(obs_atol()[0])
    if variant in ("TT", "T4"):
        xs = [X_HALF[0], X_END[0], NET_X[0], NET_X[1], hx]
        if variant == "T4":
            xs += [X_HALF[1], X_END[1], float(f32(cfg.humanoid2_root_pos[0]) + BACK)]
        bad = (near(bx, xs, pos) & moving_x) | (near(by, [Y_BOUNCE, -Y_BOUNCE, NET_Y, -NET_Y], pos) & moving_y)
        bad |= near(bz, [Z_BOUNCE, NET_Z[0], NET_Z[1], Z_DIE], pos) | (near(vx, [0.0], vel) & moving_x)
    elif variant == "T3":
        bad = (np.abs(bx - (px - float(T3_PADDLE_BACK))) <= pos(px.max()) + body) | near(bz, [Z_DIE], pos) | (near(vx, [0.0], vel) & moving_x)
    else:
        bad = (near(bx, [hx], pos) & moving_x) | (np.abs(bx - (px - float(TN_PADDLE_BACK))) <= pos(px.max()) + body)
        bad |= near(bz, [Z_DIE], pos) | (near(vx, [0.0, TN_HIT_VX], vel) & moving_x)
    bad |= near(t["pre_vx"].astype(np.float64), [0.0], vel) & (t["pre_vx"] != 0)
    return bad & t["known"]


# ------------------------------------------------------------------------------------------------------------------ the reference trajectory
@functools.lru_cache(maxsize=None)
def oracle_run(variant, n, seed, resets=False):
    """The reference trajectory of `scenarios(variant, n, seed, resets)`: STEPS oracle steps.  -> namespace(cfg, probe, steps, meta, num_agents,
    tables); a step is a dict: st (the oracle's state blob at its start), act, flags0, main (snapshot of the oracle after it), terms, near, keep
    (neither SensitivityProbe nor near_threshold set it aside), cells, edge (zeros: ball_contact_scenarios.compare_step's plain tolerances).
    Computed once per key and shared by the tests; nothing in it is to be written to."""
    from oracle import binding
    binding.build()
    blob, act, meta = scenarios(variant, n, seed, resets)
    cfg = scene.build_config(variant, num_envs=n, seed=ENV_SEED)
    A = cfg.num_humanoids
    o, watch, parked = (binding.OracleEnv(c, threads=8) for c in (cfg, never_times_out(cfg), never_times_out(cfg)))
    probe = SensitivityProbe(binding, cfg)
    o.set_state(blob)
    steps = []
    for _ in range(STEPS):
        st = o.get_state()
        ball0, rb0, flags0, progress0 = np.array(o.ball), o.refresh_rigid_body_states().astype(np.float64), np.array(o.flags), np.array(o.progress_buf)
        o.step(act)
        main = sc.snapshot(o)
        watch.set_state(st)
        watch.step(act)
        parked.set_state(st)
        parked.ball[0:3] = np.array([[10.0], [10.0], [5.0]])
        parked.ball[7:13] = 0.0
        parked.step(act)
        assert not parked.reset_buf.any()
        w = sc.snapshot(watch)
        t = terms(cfg, ball0, rb0, w, parked.refresh_rigid_body_states())
        t["watch_rb"] = watch.refresh_rigid_body_states()
        near = near_threshold(cfg, t)
        # The probe's jitter moves an exactly placed coordinate off its threshold, which the step itself cannot: in a free flight (no contact switch) with
        # the coordinate's velocity exactly zero the env-step is judged by near_threshold alone, which looks at the coordinates that do move.
        exact = t["free_flight"] & t["known"] & (((t["pre_vx"] == 0) & (t["vx"] == 0)) | (t["vy0"] == 0)) & meta["exact"]
        keep = ~near & (~probe.sensitive(st, act, o) | exact)
        after = progress0.reshape(n, A)[:, 0] + 1
        cells = classify(cfg, t, flags0, after, resets)
        assert sorted(cells) == sorted(cells_of(variant, resets))
        steps.append(dict(st=st, act=act, flags0=flags0, progress_after=after, main=main, watch=w, terms=t, near=near, keep=keep, cells=cells, edge=np.zeros(n)))
    for x in (o, watch, parked):
        x.close()
    return types.SimpleNamespace(cfg=cfg, probe=probe, steps=steps, meta=meta, num_agents=A, tables=None, resets=resets)


def cell_counts(run, kept=True, only_timeouts=False):
    """-> {cell: env-steps in it} over the kept env-steps (kept=False: all); only_timeouts: over those that time out in that step."""
    L = int(run.cfg.max_episode_length)
    counts = dict.fromkeys(run.steps[0]["cells"], 0)
    for s in run.steps:
        k = s["keep"] | (not kept)
        if only_timeouts:
            k = k & (s["progress_after"] >= L - 1)
        for name, mask in s["cells"].items():
            counts[name] += int((mask & k).sum())
    return counts


def tolerances(cfg):
    return sc.tolerances(cfg)
