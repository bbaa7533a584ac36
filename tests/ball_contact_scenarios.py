"""Scripted states that put the 7-dof (TT / TN / T3) and the 4-actor (T4) step on every branch of the ball's contact code (DESIGN.md §3
step 2.4: ground plane, table slab, net slab, paddle disc, six capsule / sphere shapes per humanoid, the broad phase), and the
oracle-only book-keeping of the tests that use them (tests/test_ball_contacts_host.py / _gpu.py).

The random-action rollouts reach most of these branches by a handful of env-steps out of half a million, and some never.  `scenarios`
starts every env from the variant's created state, gives the arm(s) a drawn pose inside the limits (held by the actions whose PD target
it is) and, in half the envs, drawn joint velocities, and AIMS the ball: it flies freely (`launch`: the oracle's semi-implicit Euler
backwards) so that in step (env % 7) % 3 of STEPS, at a drawn micro-step, it is where the case wants it relative to the body — which for
a link-attached body is where a first oracle pass with the ball parked far away finds that link at the start of that step.  Cases that
cannot be flown into (the ball's centre inside a slab or the blade, a given penetration depth) are placed in step 0.  The group is
env % G (ground, table, net, paddle, shapes, broad phase; for T4 the last three again on humanoid 2); inside a group the case cycles with
the env's index, so that every cell of `cells_of(variant)` gets its share of the envs whatever the seed.

Everything here is decided from the ORACLE and the config, never from a kernel's output:
  * a contact CLASS is reached at an env-step when the main oracle's result (ball position / velocity / spin, rewards, reset, flags) differs
    by more than 100 x the comparison tolerance from that of a counterfactual oracle stepped from the same state whose Config has that body
    taken away (`counterfactual_configs`).  The oracle reads all of it from its config; the product library is never built from such a config.
  * the SUB-CASE (which face, edge, end cap, which side of the bounce threshold ...) is plain fp64 geometry of this module on the oracle's
    pre-step state and refresh_rigid_body_states(): the ball flies freely to the first micro-step at which some body's separation is below
    contact_offset, bodies move linearly with the velocities they have at the step's start; an env-step counts for a sub-case only when that
    body is the only one active there.  The cells in which the specification says NOTHING happens (separating inside the offset zone, the
    broad-phase cells) are geometry alone, and there the counterfactual must agree with the main run exactly.
In the variants that end the episode below z = 0.1 (all but TN) a ball on the ground resets in the same step: what shows of the contact is
the reward alpha |vx| of a ball whose vx the friction impulse turns from negative to positive (spin about +y keeps it slipping), and the
push out of the ground does not show at all — the slab and the blade carry the depenetration cells there."""
import functools
import types

import numpy as np

from helpers import BALL_ROWS, RTOL, SCALES, SensitivityProbe, assert_close, mask_envs, obs_atol, reward_atol
from isaacgym_amd import scene

STEPS = 3
FLOOR = 8                    # kept env-steps every cell must reach, per variant
ENV_SEED = 11                # the config seed of the oracle and of the env under test
EXCLUDED_BOUND = 0.02        # as the scripted 27-dof suite (tests/ta_branch_scenarios.py)
REACHED = 100.0              # x the comparison tolerance: main vs counterfactual oracle
SHAPES = ("hand", "forearm", "upper_arm", "torso", "pelvis", "head")        # scene.build_config's order
MOVING_CAPSULE, STATIC_CAPSULE = 1, 3
FIELDS = ("dof_pos", "dof_vel", "dof_force", "ball", "flags", "episode", "progress_buf", "reset_buf", "rew_buf", "obs_buf")

# Edge, corner and rim cells: the contact normal is (centre - closest point) / r with r = 0.02 m, so the fp32 quantum 2^-24 |x| (half an
# ulp) of a ball coordinate x turns into 2^-24 |x| / r of normal and, through jn n = (1 + e) |vn| n, into (1 + e) 2^-24 |x| / r |v_rel| of
# rebound velocity (test_gentle_policy_single_step_is_tight: 5e-4 m/s at 8 m/s).  The bound used: EDGE_FACTOR 2^-23 |x|_max / r |v_rel|,
# EDGE_FACTOR = 4 for (1 + e) <= 2 halves of an ulp on each of up to three coordinates plus the rounding of the kernel's own subtraction
# centre - closest point, which is one more ulp of |x|.  The spin takes the tangential part of the same impulse / (kappa r).
EDGE_FACTOR = 4.0

_ARM_CELLS = (["paddle/front", "paddle/back", "paddle/rim", "paddle/inside", "paddle/wrist_moving"] + [f"shape/{s}" for s in SHAPES] +
              [f"capsule/{k}_{w}" for k in ("moving", "static") for w in ("interior", "end0", "end1")] + ["shape/sphere", "shape/degenerate_centre"] +
              ["broad/inside_bound", "broad/outside_bound", "broad/in_shape_sphere_no_contact"])
_SCENE_CELLS = (["ground/above_threshold", "ground/below_threshold", "ground/separating_in_offset_zone", "ground/cap_binding", "ground/cap_free",
                 "table/top_slip", "table/top_stick", "table/pure_normal", "table/long_edge", "table/corner", "table/underside",
                 "table/inside_exit_x", "table/inside_exit_y", "table/inside_exit_z",
                 "net/face_pos_x", "net/face_neg_x", "net/top_edge", "net/inside"])
NO_EFFECT = ("ground/separating_in_offset_zone", "broad/inside_bound", "broad/outside_bound", "broad/in_shape_sphere_no_contact")
EDGE_CELLS = ("table/long_edge", "table/corner", "net/top_edge", "paddle/rim")
# The ball's centre ON a sphere's centre is a discontinuity by construction (any jitter gives another normal): SensitivityProbe sets every such
# env-step aside, and check_excluded holds the kernel to the oracle's main run there (a jittered run has a normal of its own).  Its floor
# counts the env-steps reached, all of which go through check_excluded.
PROBED_CELLS = ("shape/degenerate_centre",)


def cells_of(variant):
    return _SCENE_CELLS + _ARM_CELLS + ([f"h2/{c}" for c in _ARM_CELLS] if variant == "T4" else [])


CELLS = {v: cells_of(v) for v in ("TT", "TN", "T3", "T4")}


# ------------------------------------------------------------------------------------------------------------------ small fp64 helpers
def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _quat_rot(q):
    """xyzw [n,4] -> [n,3,3]"""
    x, y, z, w = (q[:, i] for i in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def _mv(R, v):
    return np.einsum("nij,nj->ni", R, np.broadcast_to(v, (R.shape[0], 3)))


def _micro(cfg):
    per = cfg.substeps * cfg.ball_substeps
    return per, float(cfg.dt) / per


def launch(cfg, target, vel_at_test, m):
    """-> (start position, start velocity): a ball started there is at `target` [n,3] at the contact test of micro-step m [n] (counted from
    the start; per micro-step the oracle kicks v.z by g hb, tests the contacts, then moves p by v hb) with velocity `vel_at_test`."""
    _, hb = _micro(cfg)
    g, m = float(cfg.gravity_z), np.asarray(m, np.float64)
    v0 = np.array(vel_at_test, np.float64)
    v0[:, 2] -= g * hb * (m + 1)
    p0 = np.asarray(target, np.float64) - v0 * (m * hb)[:, None]
    p0[:, 2] -= g * hb * hb * m * (m + 1) / 2
    return p0, v0


class Arm:
    """World geometry of humanoid `arm`'s paddle and shapes at the start of a step, from the config and refresh_rigid_body_states():
    row 40 arm + 31 + j is chain link j (pose, linear and angular velocity of its origin)."""

    def __init__(self, cfg, rb, arm):
        rb = np.asarray(rb, np.float64)
        n = rb.shape[0]
        self.n, self.cfg = n, cfg
        rows = rb[:, scene.NUM_HUMANOID_BODIES * arm + 31: scene.NUM_HUMANOID_BODIES * arm + 38]
        self.p, self.v, self.w = rows[:, :, 0:3], rows[:, :, 7:10], rows[:, :, 10:13]
        self.R = np.stack([_quat_rot(rows[:, j, 3:7]) for j in range(7)], axis=1)
        self.base_R = np.array(list(cfg.base2_rot if arm else cfg.base_rot), np.float64).reshape(3, 3)
        self.bound = np.array(list(cfg.humanoid2_bound_center if arm else cfg.humanoid_bound_center), np.float64)
        self.shapes = cfg.shape2 if arm else cfg.shape
        L = cfg.paddle_link
        self.pc, self.vpc = self.point(L, list(cfg.paddle_center))
        self.pn = _mv(self.R[:, L], np.array(list(cfg.paddle_normal), np.float64))
        self.pnd = np.cross(self.w[:, L], self.pn)

    def point(self, link, local):
        local = np.array(local, np.float64)
        if link < 0:
            return np.broadcast_to(local, (self.n, 3)).copy(), np.zeros((self.n, 3))
        off = _mv(self.R[:, link], local)
        return self.p[:, link] + off, self.v[:, link] + np.cross(self.w[:, link], off)

    def shape(self, s):
        sh = self.shapes[s]
        (a, va), (b, vb) = self.point(sh.link, list(sh.a)), self.point(sh.link, list(sh.b))
        return a, va, b, vb, float(sh.radius)

    def paddle_at(self, t):
        t = np.asarray(t, np.float64).reshape(-1, 1) * np.ones((self.n, 1))
        return self.pc + self.vpc * t, _unit(self.pn + self.pnd * t)


# ------------------------------------------------------------------------------------------------------------------ the scripted states
def _tables(variant, n, rng, clamp):
    """The randomisation tables of the GPU cases: test_gpu_parity._dr_tables, with restitution_scale in [1.3, 1.6] where `clamp` [n] (the
    paddle and shape groups: 0.8 x 1.3 > restitution_max = 1, the clamp binds) and in (0, 0.7) elsewhere."""
    u = lambda lo, hi, shape: rng.uniform(lo, hi, shape).astype(np.float32)
    es = np.where(clamp, u(1.3, 1.6, n), u(0.0, 0.7, n)).astype(np.float32)
    return dict(dof_stiffness_scale=u(0.5, 1.5, (7, n)), dof_damping_scale=u(0.5, 1.5, (7, n)), link_mass_scale=u(0.5, 1.5, (7, n)),
                restitution_scale=es, friction_scale=u(0.7, 1.3, n))


DR_NOISE = dict(action_noise_sigma=0.02, observation_noise_sigma=0.002)


# the group of env e is GROUP_CYCLE[e % G]: 0 ground, 1 table, 2 net, 3 paddle, 4 shapes, 5 broad phase, 6 - 8 the last three on humanoid 2.  The
# shapes group has the most cases (17 shares) and the ones most often spoilt by a neighbouring body, so it holds three slots of the cycle;
# G = 8 / 13 shares no factor with the 7 of the step rule.
GROUP_CYCLE = {False: (0, 1, 2, 3, 4, 5, 4, 4), True: (0, 1, 2, 3, 4, 5, 6, 7, 8, 4, 7, 4, 7)}


def groups_of(variant, n):
    """-> (group [n], case [n]: the running index of the env inside its group)."""
    cycle = np.array(GROUP_CYCLE[variant == "T4"])
    G, env = len(cycle), np.arange(n)
    rank = np.array([int((cycle[:i] == cycle[i]).sum()) for i in range(G)])
    mult = np.array([int((cycle == g).sum()) for g in cycle])
    return cycle[env % G], (env // G) * mult[env % G] + rank[env % G]


def dr_tables(variant, n, seed):
    group, _ = groups_of(variant, n)
    return _tables(variant, n, np.random.default_rng([seed, 77]), np.isin(group, (3, 4, 6, 7)))


def scenarios(variant, n, seed, dr=False):
    """-> (state blob of the oracle at the start, actions [n A, 7] held over the STEPS steps, meta: group / kind / when [n])."""
    from oracle import binding
    binding.build()
    cfg = scene.build_config(variant, num_envs=n, seed=ENV_SEED)
    o = binding.OracleEnv(cfg, threads=8)
    if dr:
        o.set_randomization(**dr_tables(variant, n, seed), **DR_NOISE)
    A = cfg.num_humanoids
    per, hb = _micro(cfg)
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    pm = lambda: rng.choice([-1.0, 1.0], n)
    deg = np.pi / 180
    env = np.arange(n)
    (group, case), when = groups_of(variant, n), (env % 7) % 3
    arm_of = np.where(group >= 6, 1, 0)
    agroup = np.where(group >= 6, group - 3, group)          # 3 paddle, 4 shapes, 5 broad phase on either humanoid
    r, off = float(cfg.ball_radius), float(cfg.contact_offset)
    cap = float(cfg.max_depenetration_velocity) * hb

    kind = np.zeros(n, np.int64)
    for gi, k in {0: 5, 1: 9, 2: 4, 3: 4, 4: 17, 5: 3}.items():
        kind = np.where(agroup == gi, case % k, kind)
    # the shapes group has 17 shares: the cases most often spoilt by a neighbouring body get more than one (the forearm's elbow end cap three, its
    # interior, its wrist end cap and the upper arm two each)
    kind = np.where(agroup == 4, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 2, 2, 4, 13, 6, 1, 3])[kind % 17], kind)

    # ---- the arms: a pose strictly inside the limits, held by the actions; half the envs at rest
    lo, hi = (np.array([getattr(cfg.joint[j], k) for j in range(7)], np.float64) for k in ("lower", "upper"))
    q = rng.uniform(-0.5, 0.5, (A, 7, n))
    moving = rng.random(n) < 0.5
    qd = rng.uniform(-2.0, 2.0, (A, 7, n)) * moving
    for a in range(A):
        wrist = moving & (agroup == 3) & (arm_of == a)        # the blade's surface velocity term cross(cross(nn, nd), closest - cc)
        qd[a, 4:7, wrist] = (rng.uniform(3.0, 8.0, (3, n)) * rng.choice([-1.0, 1.0], (3, n)))[:, wrist].T
        end0 = (agroup == 4) & (arm_of == a) & (kind == 2)
        q[a, 3, end0] = u(-1.0, -0.6)[end0]                   # the forearm folded up: its elbow end cap is clear of the upper arm
    if variant == "T3":       # T3 ends the episode when the ball is behind the paddle in x (T3:1146), and a reset hides the contact: the arm
        back = agroup == 4    # swung back, the shapes are hit from the front with the paddle behind them
        q[0, 0, back] = u(1.3, 2.0)[back]
        fold = back & (kind == 2)                        # (elbow end cap: the folded forearm must still point backwards, pitch + elbow > pi / 2)
        q[0, 0, fold], q[0, 3, fold] = u(2.45, 2.6)[fold], u(-0.8, -0.6)[fold]
    q = np.clip(q, (lo + 0.01)[None, :, None], (hi - 0.01)[None, :, None])
    actions = np.clip((q - 0.5 * (hi + lo)[None, :, None]) / (0.5 * (hi - lo))[None, :, None], -1, 1)
    actions = np.ascontiguousarray(actions.transpose(2, 0, 1).reshape(n * A, 7), np.float32)
    o.dof_pos[:], o.dof_vel[:] = q.reshape(A * 7, n), qd.reshape(A * 7, n)
    o.ball[0:3] = np.array([[10.0], [10.0], [5.0]])
    o.ball[7:13] = 0.0
    start = o.get_state()
    rbs = []
    for t in range(STEPS):                                    # first pass, the ball parked: where the links are at the start of each step
        rbs.append(o.refresh_rigid_body_states().astype(np.float64))
        o.step(actions)
        assert not o.reset_buf.any()

    # ---- which cases are placed in step 0 instead of flown in
    direct = np.zeros(n, bool)
    direct |= (agroup == 0) & ((variant != "TN") | np.isin(kind, (2, 3, 4)))
    direct |= (agroup == 1) & np.isin(kind, (6, 7))
    direct |= (agroup == 2) & (kind == 3)
    direct |= (agroup == 3) & (kind == 3)
    direct |= (agroup == 4) & (kind >= 13)
    when = np.where(direct, 0, when)
    mc = np.where(direct, 0, rng.integers(0, per, n))
    # Leaving the slab through z is flown INTO, at the step's last micro-step: placed at its start, the pushes of the following micro-steps bring the
    # ball to the same place whatever the first one was (s = -pz instead of -pz - r shows in one value of 12 273 along the rollouts); a ball that
    # is fast enough to go from clear of the top face to a centre below it in one micro-step gets exactly one push before the step ends.
    mc = np.where((agroup == 1) & (kind == 8), per - 1, mc)
    tc = mc * hb
    rb = np.stack(rbs)[when, env]
    arms = [Arm(cfg, rb, a) for a in range(A)]
    pick = lambda xs: np.where((arm_of == 1).reshape((n,) + (1,) * (xs[0].ndim - 1)), xs[-1], xs[0])

    P, V, W = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    vn = u(1.0, 4.0)                                          # approach speed along the normal, where a case does not set its own
    # (humanoid 2 stands at x = 3.5: the probe's 1e-6 jitter of the ball's x is 3.5e-6 m there, which over a normal of length 0.055 m (hand) or 0.02 m (rim)
    #  moves a fast rebound by more than the tolerance; its curved bodies are met slowly)
    vn = np.where((arm_of == 1) & (agroup == 4), u(0.3, 0.7), np.where((arm_of == 1) & (agroup == 3) & (kind == 2), u(0.3, 0.6), vn))
    sc_ = lambda speed: off - u(0.15, 0.85) * speed * hb      # separation at the activating micro-step: outside the zone one micro-step earlier

    def tangent(d, lo_, hi_):
        t = _unit(np.cross(d, _unit(rng.normal(size=(n, 3)))))
        return t * u(lo_, hi_)[:, None]

    # ---- ground
    m_ = agroup == 0
    gmu, ge = float(cfg.ground_friction), float(cfg.ground_restitution)
    sp = np.where(kind == 1, u(0.04, 0.14), u(0.5, 2.0))
    s = np.select([kind <= 1, kind == 2, kind == 3], [off - u(0.15, 0.85) * sp * hb, u(0.2, 0.8) * off, -cap * u(1.1, 1.7)], -cap * u(0.1, 0.85))
    vz = np.where(kind == 2, u(0.05, 1.0), -sp)
    turn = gmu * (1.0 + np.where(sp > cfg.bounce_threshold, ge, 0.0)) * sp
    tn = variant == "TN"
    P[m_] = np.stack([u(0.7, 2.8), u(-0.6, 0.6), float(cfg.ground_z) + r + s], 1)[m_]
    V[m_] = np.stack([u(-2, 2) if tn else -u(0.15, 0.6) * turn, u(-0.3, 0.3), vz], 1)[m_]
    W[m_] = np.stack([u(-20, 20), u(-50, 50) if tn else u(300, 420), u(-20, 20)], 1)[m_]

    # ---- table slab and net slab
    for gi, box in ((1, cfg.table), (2, cfg.net)):
        c, h = np.array(list(box.center), np.float64), np.array(list(box.half), np.float64)
        m_ = agroup == gi
        top = c[2] + h[2]
        if gi == 1:
            x = c[0] + np.where(rng.random(n) < 0.5, -u(0.15, h[0] - 0.6), u(0.15, h[0] - 0.1))     # clear of the net and of humanoid 1's reach
            y = c[1] + u(-1, 1) * (h[1] - 0.1)
            sx, sy, th = pm(), pm(), u(25, 65) * deg
            ang = u(0, 2 * np.pi)
            # (a corner's normal takes the quantum of all three coordinates: at the far end, x = 3.12, the probe's 1e-6 jitter moves a 1 m/s rebound
            #  by more than the tolerance; the corners used are the near end's, x = 0.38, at 0.3 - 0.8 m/s)
            sp = np.select([kind == 0, kind == 1, kind == 4], [u(1.0, 2.0), u(2.0, 4.0), u(0.3, 0.8)], vn)
            vt = np.select([kind == 0, kind == 1, kind == 2], [u(4.0, 6.0), u(0.2, 0.6), 0.0], u(0.0, 1.5))
            s = sc_(sp)
            flat = np.stack([vt * np.cos(ang), vt * np.sin(ang), 0 * vt], 1)
            edge = np.stack([0 * th, sy * np.cos(th), np.sin(th)], 1)
            corner = _unit(np.stack([-u(0.4, 1), sy * u(0.4, 1), u(0.4, 1)], 1))
            depth = u(0.001, 0.008)                           # the exit depth of a centre inside the slab: below the cap, so that s = -p - r binds it
            ins = [np.stack([sx * (h[0] - depth), u(-0.5, 0.5) * h[1], u(-0.3, 0.3) * h[2]], 1),
                   np.stack([u(-0.8, 0.8) * h[0], sy * (h[1] - depth), u(-0.3, 0.3) * h[2]], 1),
                   np.stack([x - c[0], y - c[1], h[2] - depth], 1)]
            pos = [np.stack([x, y, top + r + s], 1)] * 3 + [np.stack([x, c[1] + sy * h[1], top + 0 * x], 1) + edge * (r + s)[:, None],
                                                            (c + np.stack([-h[0] + 0 * x, sy * h[1], h[2] + 0 * x], 1)) + corner * (r + s)[:, None],
                                                            np.stack([x, y, c[2] - h[2] - r - s], 1)] + [c + d for d in ins]
            down = np.stack([0 * sp, 0 * sp, -sp], 1)
            vel = [flat + down] * 3 + [-edge * sp[:, None] + np.stack([u(-1, 1), 0 * x, 0 * x], 1), -corner * sp[:, None] + tangent(corner, 0, 0.5),
                                       flat - down] + [np.where(np.arange(3) == ax, -np.sign(d[:, ax:ax + 1]) * u(0.3, 1.0)[:, None], rng.uniform(-1, 1, (n, 3)))
                                                       for ax, d in enumerate(ins)]     # moving inwards: an impulse as well as the push
            vel[8] = np.stack([u(-1, 1), u(-1, 1), -(depth + r + u(0.002, 0.006)) / hb], 1)
            W[m_ & (kind != 2)] = rng.uniform(-30, 30, (n, 3))[m_ & (kind != 2)]
        else:
            y = c[1] + u(-1, 1) * (h[1] - 0.1)
            z = u(c[2] - h[2] + 0.035, top - 0.02)            # over the table top by more than the ball's radius
            sx, th = np.where(kind == 0, 1.0, np.where(kind == 1, -1.0, pm())), u(25, 65) * deg
            sp = np.where(kind <= 1, u(1.0, 5.0), u(0.3, 1.0))   # (the top edge at x = 1.75: as the corners)
            s = sc_(sp)
            edge = np.stack([sx * np.cos(th), 0 * th, np.sin(th)], 1)
            face = np.stack([c[0] + sx * (h[0] + r + s), y, z], 1)
            dx = u(0.1, 0.8) * h[0] * sx
            pos = [face, face, np.stack([c[0] + sx * h[0], y, top + 0 * y], 1) + edge * (r + s)[:, None], np.stack([c[0] + dx, y, z], 1)]
            into = np.stack([-sx * sp, u(-1, 1), u(-0.5, 0.5)], 1)
            vel = [into, into, -edge * sp[:, None] + np.stack([0 * y, u(-1, 1), 0 * y], 1), np.stack([-sx * u(0.3, 1.0), u(-1, 1), u(-0.5, 0.5)], 1)]
            W[m_] = rng.uniform(-30, 30, (n, 3))[m_]
        for k in range(len(pos)):
            P[m_ & (kind == k)], V[m_ & (kind == k)] = pos[k][m_ & (kind == k)], vel[k][m_ & (kind == k)]

    # ---- paddle disc (front face, back face, rim, centre inside the blade), on the humanoid of the group
    m_ = agroup == 3
    R_, tp_ = float(cfg.paddle_radius), float(cfg.paddle_half_thickness)
    L = cfg.paddle_link
    cn = [a.paddle_at(tc) for a in arms]
    C, N = pick([x[0] for x in cn]), pick([x[1] for x in cn])
    U0, Nd, R6 = pick([a.vpc for a in arms]), pick([a.pnd for a in arms]), pick([a.R[:, L] for a in arms])
    ang = u(-60, 60) * deg                                    # in the blade's plane, on the far side from the hand
    e = _mv(R6, np.array([1.0, 0, 0])) * np.cos(ang)[:, None] + _mv(R6, np.array([0, 0, 1.0])) * np.sin(ang)[:, None]
    e = _unit(e - N * _dot(e, N)[:, None])
    e2, sg, ph = np.cross(N, e), pm(), u(15, 70) * deg
    sg = np.where(kind == 0, 1.0, np.where(kind == 1, -1.0, sg))
    s = sc_(vn)
    rho = u(0.0, 0.05)
    dirn = np.where((kind == 2)[:, None], e * np.cos(ph)[:, None] + N * (sg * np.sin(ph))[:, None], N * sg[:, None])
    closest = C + np.where((kind == 2)[:, None], e * R_, e * rho[:, None]) + N * (sg * tp_)[:, None]
    hh = sg * u(0.0005, 0.004)
    inside = kind == 3
    closest = np.where(inside[:, None], C + e * rho[:, None] + N * (sg * tp_)[:, None], closest)
    surf = U0 + np.cross(np.cross(N, Nd), closest - C)
    P[m_] = np.where(inside[:, None], C + e * rho[:, None] + N * hh[:, None], closest + dirn * (r + s)[:, None])[m_]
    V[m_] = (surf + np.where(inside[:, None], -N * (sg * u(0.3, 1.0))[:, None], -dirn * vn[:, None]) + e2 * u(-2, 2)[:, None])[m_]
    W[m_] = rng.uniform(-30, 30, (n, 3))[m_]

    # ---- the six shapes: hand, forearm interior / end a / end b, upper arm, torso interior / end a / end b, pelvis, head
    m_ = agroup == 4
    which = np.array([0, 1, 1, 1, 2, 3, 3, 3, 4, 5, 0, 0, 0, 4])[kind]     # 13: the ball's centre ON the pelvis' or the head's centre, in turn
    which = np.where((kind == 13) & ((case // 17) % 2 == 1), 5, which)
    Rb = [a.base_R for a in arms]
    az = u(-20, 120) * deg                                    # static shapes: from the front and the side away from the right arm
    for si in range(6):
        geo = [a.shape(si) for a in arms]
        a0, va, b0, vb = (pick([x[i] for x in geo]) for i in range(4))
        Rs = geo[0][4]
        link = arms[0].shapes[si].link
        aw, bw = a0 + va * tc[:, None], b0 + vb * tc[:, None]
        axis = _unit(bw - aw)
        RL = pick([a.R[:, max(link, 0)] for a in arms])
        base = pick([np.broadcast_to(x, (n, 3, 3)) for x in Rb])
        front = (lambda x: x * np.where(x[:, :1] < 0, -1.0, 1.0)) if variant == "T3" else (lambda x: x)
        if si == 0:
            d, tpar = front(_unit(_mv(RL, np.array([1.0, 0, 0])) * u(-0.5, 0.2)[:, None] + _mv(RL, np.array([0, 1.0, 0])) * pm()[:, None] +
                            _mv(RL, np.array([0, 0, 1.0])) * u(-0.5, 0.5)[:, None])), 0 * az
        elif si == 1:
            psi = u(0, 2 * np.pi)
            perp = front(_mv(RL, np.array([0, 1.0, 0])) * np.cos(psi)[:, None] + _mv(RL, np.array([0, 0, 1.0])) * np.sin(psi)[:, None])
            # the elbow end cap (radius + r = 0.05 about a) lies inside the upper arm's end sphere (0.055 about its b, 0.03 away) except on the
            # side facing away from b: the ball comes from there, tilted off the forearm's axis towards (a - upper arm's b)
            ub = [x.shape(2) for x in arms]
            away = aw - (pick([x[2] for x in ub]) + pick([x[3] for x in ub]) * tc[:, None])
            side = _unit(away - axis * _dot(away, axis)[:, None])
            ph0, ph1 = u(30, 80) * deg, u(0, 60) * deg
            d = np.select([(kind == 2)[:, None], (kind == 3)[:, None]],
                          [-axis * np.cos(ph0)[:, None] + side * np.sin(ph0)[:, None], axis * np.cos(ph1)[:, None] + perp * np.sin(ph1)[:, None]], perp)
            tpar = np.select([kind == 2, kind == 3], [0.0, 1.0], u(0.25, 0.75))
        elif si == 2:
            psi = u(-80, 80) * deg
            perp = _mv(RL, np.array([1.0, 0, 0])) * np.sin(psi)[:, None] - _mv(RL, np.array([0, 1.0, 0])) * np.cos(psi)[:, None]
            d, tpar = front(_unit(perp - axis * _dot(perp, axis)[:, None])), u(0.5, 0.85)
        elif si == 3:
            perp = _mv(base, np.array([1.0, 0, 0])) * np.cos(az)[:, None] + _mv(base, np.array([0, 1.0, 0])) * np.sin(az)[:, None]
            ph = u(50, 80) * deg
            d = np.select([(kind == 6)[:, None], (kind == 7)[:, None]],
                          [-axis * np.cos(ph)[:, None] + perp * np.sin(ph)[:, None], axis * np.cos(ph)[:, None] + perp * np.sin(ph)[:, None]], perp)
            tpar = np.select([kind == 6, kind == 7], [0.0, 1.0], u(0.2, 0.8))
        else:
            el = (u(-60, 0) if si == 4 else u(0, 70)) * deg
            d = _mv(base, np.array([1.0, 0, 0])) * (np.cos(az) * np.cos(el))[:, None] + _mv(base, np.array([0, 1.0, 0])) * (np.sin(az) * np.cos(el))[:, None] + \
                _mv(base, np.array([0, 0, 1.0])) * np.sin(el)[:, None]
            tpar = 0 * az
        s = sc_(vn)
        cp = aw + (bw - aw) * tpar[:, None]
        sel = m_ & (which == si)
        P[sel] = (cp + d * (Rs + r + s)[:, None])[sel]
        V[sel] = (va + (vb - va) * tpar[:, None] - d * vn[:, None] + tangent(d, 0, 1.5))[sel]
        on = sel & (kind >= 13)                               # d2 = 0: the fallback normal (0, 0, 1); moving down, so that it takes an impulse too
        P[on], V[on] = aw[on], np.stack([u(-0.3, 0.3), u(-0.3, 0.3), -u(0.3, 1.0)], 1)[on]
    W[m_] = rng.uniform(-30, 30, (n, 3))[m_]

    # ---- broad phase: just inside / just outside the humanoid's bound sphere, and inside the torso's bounding sphere beyond its reach
    m_ = agroup == 5
    base = pick([np.broadcast_to(x, (n, 3, 3)) for x in Rb])
    bc = pick([np.broadcast_to(a.bound, (n, 3)) for a in arms])
    az2, el2 = u(-60, 60) * deg, u(-10, 50) * deg
    d = _mv(base, np.array([1.0, 0, 0])) * (np.cos(az2) * np.cos(el2))[:, None] + _mv(base, np.array([0, 1.0, 0])) * (np.sin(az2) * np.cos(el2))[:, None] + \
        _mv(base, np.array([0, 0, 1.0])) * np.sin(el2)[:, None]
    rad = float(cfg.humanoid_bound_radius) + np.where(kind == 0, -1.0, 1.0) * u(0.004, 0.03)
    geo = [a.shape(STATIC_CAPSULE) for a in arms]
    ta, tb = pick([x[0] for x in geo]), pick([x[2] for x in geo])
    perp = _mv(base, np.array([1.0, 0, 0])) * np.cos(az)[:, None] + _mv(base, np.array([0, 1.0, 0])) * np.sin(az)[:, None]
    near = ta + (tb - ta) * u(0.35, 0.65)[:, None] + perp * u(0.14, 0.19)[:, None]
    P[m_] = np.where((kind == 2)[:, None], near, bc + d * rad[:, None])[m_]
    V[m_] = np.where((kind == 2)[:, None], _unit(tb - ta) * u(-1, 1)[:, None], tangent(d, 0.3, 1.0))[m_]

    p0, v0 = launch(cfg, P, V, when * per + mc)
    o.set_state(start)
    o.ball[0:3], o.ball[7:10], o.ball[10:13] = p0.T, v0.T, W.T
    blob = o.get_state()
    o.close()
    return blob, actions, dict(group=group, kind=kind, when=when, arm=arm_of)


# ------------------------------------------------------------------------------------------------------------------ counterfactual configs
def _copy(cfg):
    return scene.Config.from_buffer_copy(cfg)


def counterfactual_configs(cfg):
    """{class: Config with that body taken away}.  Only the oracle is ever built from these."""
    out = {}
    c = _copy(cfg); c.ground_z = -100.0; out["ground"] = c
    c = _copy(cfg); c.table.center[2] = -100.0; out["table"] = c
    c = _copy(cfg); c.net.center[2] = -100.0; out["net"] = c
    c = _copy(cfg); c.paddle_radius, c.paddle_half_thickness = 1e-9, 1e-9; c.paddle_center[2] = 100.0; out["paddle"] = c
    for arm in range(cfg.num_humanoids):
        for s, name in enumerate(SHAPES):
            c = _copy(cfg)
            sh = (c.shape2 if arm else c.shape)[s]
            sh.radius = 1e-9
            for k in range(3):
                sh.a[k], sh.b[k] = (0.0, 0.0, 100.0 if sh.link >= 0 else -100.0)[k], (0.0, 0.0, 100.0 if sh.link >= 0 else -100.0)[k]
            out[("h2/" if arm else "") + name] = c
    return out


def snapshot(o):
    s = types.SimpleNamespace(**{k: np.array(getattr(o, k)) for k in FIELDS})
    s.num_agents = o.num_agents
    return s


def _differs(a, b, ra, A, factor):
    """bool [n]: the results a / b of two oracles differ by more than factor x the comparison tolerance (factor 0: at all)."""
    n = a.ball.shape[1]
    bad = (a.reset_buf != b.reset_buf).reshape(n, A).any(1) | (a.flags != b.flags).reshape(-1, n).any(0)
    for name, rows in BALL_ROWS.items():
        if name != "ball_quat":
            x, y = a.ball[rows].astype(np.float64), b.ball[rows].astype(np.float64)
            bad |= (np.abs(x - y) > factor * (RTOL * SCALES[name] + RTOL * np.abs(y))).any(0)
    x, y = a.rew_buf.astype(np.float64), b.rew_buf.astype(np.float64)
    bad |= (np.abs(x - y) > factor * (ra + RTOL * np.abs(y))).reshape(n, A).any(1)
    return bad


# ------------------------------------------------------------------------------------------------------------------ fp64 geometry of the sub-cases
def _resolve_terms(cfg, v, w, nrm, usurf):
    vrel = v + np.cross(w, -float(cfg.ball_radius) * nrm) - usurf
    vn = _dot(vrel, nrm)
    return vrel, vn, np.linalg.norm(vrel - nrm * vn[:, None], axis=1)


def _box(cfg, box, p):
    c, h = np.array(list(box.center), np.float64), np.array(list(box.half), np.float64)
    d = p - c
    diff = d - np.clip(d, -h, h)
    dist = np.linalg.norm(diff, axis=1)
    inside = dist == 0.0
    pen = h - np.abs(d)
    ax = np.argmin(pen, axis=1)
    n_in = np.zeros_like(d)
    n_in[np.arange(len(d)), ax] = np.where(d[np.arange(len(d)), ax] >= 0, 1.0, -1.0)
    nrm = np.where(inside[:, None], n_in, diff / np.maximum(dist, 1e-300)[:, None])
    s = np.where(inside, -pen[np.arange(len(d)), ax], dist) - float(cfg.ball_radius)
    return dict(s=s, n=nrm, u=np.zeros_like(d), inside=inside, exit_axis=ax, outside_axes=(diff != 0).sum(1), face_axis=np.argmax(np.abs(diff), axis=1),
                face_sign=np.sign(diff[np.arange(len(d)), np.argmax(np.abs(diff), axis=1)]))


def _capsule(cfg, p, a, b, va, vb, radius):
    ab = b - a
    l2 = _dot(ab, ab)
    sphere = l2 <= 1e-12
    t = np.where(sphere, 0.0, np.clip(_dot(p - a, ab) / np.where(sphere, 1.0, l2), 0.0, 1.0))
    diff = p - (a + ab * t[:, None])
    dist = np.linalg.norm(diff, axis=1)
    on = dist <= 1e-12
    nrm = np.where(on[:, None], np.array([0.0, 0.0, 1.0]), diff / np.maximum(dist, 1e-300)[:, None])
    return dict(s=dist - radius - float(cfg.ball_radius), n=nrm, degenerate=on, u=va + (vb - va) * t[:, None], t=t, sphere=sphere,
                in_sphere=np.linalg.norm(p - 0.5 * (a + b), axis=1) < 0.5 * np.sqrt(l2) + radius + float(cfg.ball_radius) + float(cfg.contact_offset))


def _disc(cfg, p, C, N, U0, Nd):
    R_, tp_ = float(cfg.paddle_radius), float(cfg.paddle_half_thickness)
    d = p - C
    hgt = _dot(d, N)
    radial = d - N * hgt[:, None]
    rr = np.linalg.norm(radial, axis=1)
    inside = (np.abs(hgt) < tp_) & (rr < R_)
    sg = np.where(hgt >= 0, 1.0, -1.0)
    closest = C + N * np.clip(hgt, -tp_, tp_)[:, None] + radial * (np.minimum(rr, R_) / np.maximum(rr, 1e-300))[:, None]
    closest = np.where(inside[:, None], C + N * (sg * tp_)[:, None] + radial, closest)
    diff = p - closest
    dist = np.linalg.norm(diff, axis=1)
    nrm = np.where(inside[:, None], N * sg[:, None], diff / np.maximum(dist, 1e-300)[:, None])
    spin_term = np.cross(np.cross(N, Nd), closest - C)
    return dict(s=np.where(inside, -(tp_ - np.abs(hgt)), dist) - float(cfg.ball_radius), n=nrm, u=U0 + spin_term, inside=inside, rim=rr > R_, sg=sg,
                spin_speed=np.linalg.norm(spin_term, axis=1))


def first_contact(cfg, ball, rb):
    """Free flight of the ball from the pre-step state to the first micro-step at which a body's separation is below contact_offset.
    -> {body: dict of its terms there (+ active, sole: bool [n])}, found [n]; bodies: ground, table, net, paddle, the SHAPES, and h2/..."""
    per, hb = _micro(cfg)
    A, n = cfg.num_humanoids, ball.shape[1]
    p, v, w = (np.array(ball[rows].T, np.float64) for rows in (slice(0, 3), slice(7, 10), slice(10, 13)))
    arms = [Arm(cfg, rb, a) for a in range(A)]
    damp = max(1.0 - float(cfg.ball_angular_damping) * hb, 0.0)
    found, rec = np.zeros(n, bool), {}
    inside_bound = [np.ones(n, bool) for _ in range(A)]
    for m in range(per):
        t = m * hb
        v[:, 2] += float(cfg.gravity_z) * hb
        w = w * damp
        bodies = {"ground": dict(s=p[:, 2] - float(cfg.ground_z) - float(cfg.ball_radius), n=np.tile([0.0, 0, 1.0], (n, 1)), u=np.zeros((n, 3))),
                  "table": _box(cfg, cfg.table, p), "net": _box(cfg, cfg.net, p)}
        for a, arm in enumerate(arms):
            pre = "h2/" if a else ""
            near = np.linalg.norm(p - arm.bound, axis=1) < float(cfg.humanoid_bound_radius)
            inside_bound[a] &= near
            C, N = arm.paddle_at(t)
            bodies[pre + "paddle"] = _disc(cfg, p, C, N, arm.vpc, arm.pnd)
            for s_, name in enumerate(SHAPES):
                a0, va, b0, vb, radius = arm.shape(s_)
                bodies[pre + name] = _capsule(cfg, p, a0 + va * t, b0 + vb * t, va, vb, radius)
            for name in ["paddle"] + list(SHAPES):
                bodies[pre + name]["s"] = np.where(near, bodies[pre + name]["s"], np.inf)
        active = {k: b["s"] < float(cfg.contact_offset) for k, b in bodies.items()}
        count = np.sum(list(active.values()), axis=0)
        newly = ~found & (count > 0)
        for k, b in bodies.items():
            b["vrel"], b["vn"], b["vt"] = _resolve_terms(cfg, v, w, b["n"], b["u"])
            b["active"], b["sole"] = active[k] & newly, active[k] & newly & (count == 1)
            b["coord"], b["micro"] = np.abs(p).max(axis=1), np.full(n, m)
            if k not in rec:
                rec[k] = {kk: np.array(vv) for kk, vv in b.items()}
            else:
                for kk, vv in b.items():
                    rec[k][kk] = np.where(newly.reshape((n,) + (1,) * (np.ndim(vv) - 1)), vv, rec[k][kk])
            if m == 0:
                rec[k]["in_sphere_all"] = np.array(b.get("in_sphere", np.zeros(n, bool)))
            elif "in_sphere" in b:
                rec[k]["in_sphere_all"] &= b["in_sphere"]
        found |= newly
        p = p + v * hb
    for k in rec:
        rec[k]["active"], rec[k]["sole"] = rec[k]["active"] & found, rec[k]["sole"] & found
    return rec, found, inside_bound, p


def classify(cfg, ball0, rb0, reached, same):
    """-> ({cell: bool [n]}, edge tolerance [n]) of one env-step.  ball0 / rb0: the oracle's ball [13, n] and refresh_rigid_body_states() at the
    step's start; reached[cls] / same[cls]: the counterfactual oracle without body `cls` differs by more than REACHED x the tolerance / not at all."""
    rec, found, inside_bound, p_end = first_contact(cfg, ball0, rb0)
    n = ball0.shape[1]
    r, off = float(cfg.ball_radius), float(cfg.contact_offset)
    _, hb = _micro(cfg)
    cap, thr = float(cfg.max_depenetration_velocity) * hb, float(cfg.bounce_threshold)
    kappa = float(cfg.ball_inertia_factor)
    c = {}
    g = rec["ground"]
    hit = g["sole"] & reached["ground"]
    c["ground/above_threshold"] = hit & (g["vn"] < 0) & (-g["vn"] > thr)
    c["ground/below_threshold"] = hit & (g["vn"] < 0) & (-g["vn"] <= thr)
    c["ground/cap_binding"] = hit & (g["s"] < 0) & (-g["s"] > cap)
    c["ground/cap_free"] = hit & (g["s"] < 0) & (-g["s"] <= cap)
    c["ground/separating_in_offset_zone"] = g["sole"] & (g["s"] > 0) & (g["vn"] >= 0) & same["ground"]
    t = rec["table"]
    hit = t["sole"] & reached["table"]
    top = hit & ~t["inside"] & (t["outside_axes"] == 1) & (t["face_axis"] == 2) & (t["face_sign"] > 0) & (t["vn"] < 0)
    e_eff = np.where(-t["vn"] > thr, float(cfg.table.restitution), 0.0)
    slips = float(cfg.table.friction) * (1 + e_eff) * -t["vn"] < t["vt"] / (1 + 1 / kappa)
    c["table/top_slip"], c["table/top_stick"] = top & slips & (t["vt"] > 1e-9), top & ~slips & (t["vt"] > 1e-9)
    c["table/pure_normal"] = top & (t["vt"] <= 1e-9)
    c["table/long_edge"] = hit & ~t["inside"] & (t["outside_axes"] == 2) & (np.abs(t["n"][:, 0]) == 0)
    c["table/corner"] = hit & ~t["inside"] & (t["outside_axes"] == 3)
    c["table/underside"] = hit & ~t["inside"] & (t["outside_axes"] == 1) & (t["face_axis"] == 2) & (t["face_sign"] < 0)
    for ax, name in enumerate("xyz"):
        c[f"table/inside_exit_{name}"] = hit & t["inside"] & (t["exit_axis"] == ax)
    k = rec["net"]
    hit = k["sole"] & reached["net"]
    face = hit & ~k["inside"] & (k["outside_axes"] == 1) & (k["face_axis"] == 0)
    c["net/face_pos_x"], c["net/face_neg_x"] = face & (k["face_sign"] > 0), face & (k["face_sign"] < 0)
    c["net/top_edge"] = hit & ~k["inside"] & (k["outside_axes"] == 2) & (k["n"][:, 1] == 0) & (k["n"][:, 2] > 0)
    c["net/inside"] = hit & k["inside"]
    edge = np.zeros(n)
    for a in range(cfg.num_humanoids):
        pre = "h2/" if a else ""
        d = rec[pre + "paddle"]
        hit = d["sole"] & reached["paddle"]
        flat = hit & ~d["inside"] & ~d["rim"]
        c[pre + "paddle/front"], c[pre + "paddle/back"] = flat & (d["sg"] > 0), flat & (d["sg"] < 0)
        c[pre + "paddle/rim"], c[pre + "paddle/inside"] = hit & ~d["inside"] & d["rim"], hit & d["inside"]
        c[pre + "paddle/wrist_moving"] = hit & (d["spin_speed"] > 0.1)
        sphere, degenerate = np.zeros(n, bool), np.zeros(n, bool)
        for s_, name in enumerate(SHAPES):
            b = rec[pre + name]
            hit = b["sole"] & reached[pre + name]
            c[pre + f"shape/{name}"] = hit
            sphere |= hit & b["sphere"]
            degenerate |= hit & b["degenerate"]
            which = {MOVING_CAPSULE: "moving", STATIC_CAPSULE: "static"}.get(s_)
            if which:
                c[pre + f"capsule/{which}_interior"] = hit & (b["t"] > 0) & (b["t"] < 1)
                c[pre + f"capsule/{which}_end0"], c[pre + f"capsule/{which}_end1"] = hit & (b["t"] == 0), hit & (b["t"] == 1)
        c[pre + "shape/sphere"], c[pre + "shape/degenerate_centre"] = sphere, degenerate
        all_same = np.all([same[pre + x] for x in SHAPES] + [same["paddle"]], axis=0)
        bc = np.array(list(cfg.humanoid2_bound_center if a else cfg.humanoid_bound_center), np.float64)
        d0 = np.linalg.norm(ball0[0:3].T.astype(np.float64) - bc, axis=1)
        d1 = np.linalg.norm(p_end - bc, axis=1)
        R_ = float(cfg.humanoid_bound_radius)
        c[pre + "broad/inside_bound"] = ~found & all_same & (d0 < R_) & (d1 < R_) & (d0 > R_ - 0.05)
        c[pre + "broad/outside_bound"] = ~found & all_same & (d0 > R_) & (d1 > R_) & (d0 < R_ + 0.05)
        tor = rec[pre + SHAPES[STATIC_CAPSULE]]
        c[pre + "broad/in_shape_sphere_no_contact"] = ~found & all_same & tor["in_sphere_all"] & inside_bound[a]
    for name in EDGE_CELLS + tuple("h2/" + x for x in EDGE_CELLS if x.startswith("paddle") and cfg.num_humanoids == 2):
        b = rec[{"table": "table", "net": "net", "paddle": "paddle", "h2": "h2/paddle"}[name.split("/")[0]]]
        tol = EDGE_FACTOR * 2.0 ** -23 * b["coord"] / r * np.linalg.norm(b["vrel"], axis=1)
        edge = np.where(c[name], np.maximum(edge, tol), edge)
    return c, edge


# ------------------------------------------------------------------------------------------------------------------ the reference trajectory
@functools.lru_cache(maxsize=None)
def oracle_run(variant, n, seed, dr=False):
    """The reference trajectory of `scenarios(variant, n, seed, dr)`: STEPS oracle steps.  -> namespace(cfg, probe, tables, steps); a step is a
    dict: st (the oracle's state blob at its start), act, main (snapshot of the oracle after it), keep (~ SensitivityProbe.sensitive), cells,
    edge (the edge cells' tolerance [n], 0 elsewhere).  Computed once per key and shared by the tests; nothing in it is to be written to."""
    from oracle import binding
    binding.build()
    blob, act, meta = scenarios(variant, n, seed, dr)
    cfg = scene.build_config(variant, num_envs=n, seed=ENV_SEED)
    A = cfg.num_humanoids
    ra = (2 if A == 2 else 1) * reward_atol(cfg)
    tables = dr_tables(variant, n, seed) if dr else None

    def make(c):
        x = binding.OracleEnv(c, threads=8)
        if dr:
            x.set_randomization(**tables, **DR_NOISE)
        return x
    o = make(cfg)
    probe = SensitivityProbe(binding, cfg)
    if dr:
        probe.o2.set_randomization(**tables, **DR_NOISE)
    cf = {k: make(c) for k, c in counterfactual_configs(cfg).items()}
    o.set_state(blob)
    steps = []
    for t in range(STEPS):
        st = o.get_state()
        ball0, rb0 = np.array(o.ball), o.refresh_rigid_body_states()
        o.step(act)
        main = snapshot(o)
        reached, same = {}, {}
        for k, x in cf.items():
            x.set_state(st)
            x.step(act)
            reached[k], same[k] = _differs(x, main, ra, A, REACHED), ~_differs(x, main, ra, A, 0.0)
        keep = ~probe.sensitive(st, act, o)
        cells, edge = classify(cfg, ball0, rb0, reached, same)
        assert sorted(cells) == sorted(CELLS[variant])
        steps.append(dict(st=st, act=act, main=main, keep=keep, cells=cells, edge=edge))
    for x in cf.values():
        x.close()
    return types.SimpleNamespace(cfg=cfg, probe=probe, tables=tables, steps=steps, meta=meta, num_agents=A)


def cell_counts(run, kept=True):
    counts = dict.fromkeys(run.steps[0]["cells"], 0)
    for s in run.steps:
        for name, mask in s["cells"].items():
            counts[name] += int((mask & (s["keep"] | (not kept) | (name.replace("h2/", "") in PROBED_CELLS))).sum())
    return counts


# ------------------------------------------------------------------------------------------------------------------ the comparison
def compare_step(got, s, t, cfg, oa, ra, what):
    """A kernel's step (state view `got`) against the oracle's on the kept env-steps: the suite's integers, terms and tolerances
    (assert_state_close, obs_atol, reward_atol); the env-steps in an edge / corner / rim cell carry s["edge"] on top, on the ball's velocity,
    its spin (/ (kappa r)), the ball-velocity columns of the obs rows and the reward's alpha |vx|, and on nothing else."""
    from helpers import assert_state_close
    A, want = s["main"].num_agents, s["main"]
    for part, sel in (("face", s["keep"] & (s["edge"] == 0)), ("edge", s["keep"] & (s["edge"] > 0))):
        if not sel.any():
            continue
        g, w = mask_envs(got, sel, A), mask_envs(want, sel, A)
        tag = f"{what}, step {t}, {part} cells"
        for name in ("reset_buf", "progress_buf", "flags", "episode"):
            np.testing.assert_array_equal(getattr(g, name), getattr(w, name), err_msg=f"{tag}: {name}")
        if part == "face":
            assert_state_close(g, w, tag)
            assert_close(g.obs_buf, w.obs_buf, f"{tag}: obs", atol=oa)
            assert_close(g.rew_buf, w.rew_buf, f"{tag}: rew", atol=ra)
            continue
        extra = s["edge"][sel]
        for name in ("dof_pos", "dof_vel", "dof_force"):
            assert_close(getattr(g, name), getattr(w, name), f"{tag}: {name}", atol=RTOL * SCALES[name])
        for name, rows in BALL_ROWS.items():
            x, y = g.ball[rows], w.ball[rows]
            if name == "ball_quat":
                sign = np.sign(np.sum(x * y, axis=0, keepdims=True))
                x = x * np.where(sign == 0, 1, sign)
            more = {"ball_vel": extra, "ball_spin": extra / (float(cfg.ball_inertia_factor) * float(cfg.ball_radius))}.get(name, 0.0)
            assert_close(x, y, f"{tag}: {name}", atol=RTOL * SCALES[name] + more)
        o_tol = np.tile(oa, (g.obs_buf.shape[0], 1))
        o_tol[:, 77:80] += np.repeat(extra, A)[:, None]
        assert_close(g.obs_buf, w.obs_buf, f"{tag}: obs", atol=o_tol)
        assert_close(g.rew_buf, w.rew_buf, f"{tag}: rew", atol=ra + abs(float(cfg.alpha_velocity_reward)) * np.repeat(extra, A))


def tolerances(cfg, dr=False):
    A = cfg.num_humanoids
    return obs_atol() + (2e-6 if dr else 0.0), (2 if A == 2 else 1) * reward_atol(cfg)
