"""Scripted states that bring the ball to a MOVING 27-dof humanoid — the blade's faces and rim, the six body shapes (hand, forearm, upper arm on
links 27 / 24 / 24; torso, pelvis, head on 15 / 0 / 15), the broad-phase bound that rides on the torso — and to the scene bodies under the 27-dof
constants, and the oracle-only book-keeping of the tests that use them (tests/test_ta_ball_contacts_host.py / _gpu.py).

The contact arithmetic is shared with the 7-dof kernels and pinned by tests/ball_contact_scenarios.py; the GEOMETRY fed into it (paddle centre
velocity vpc, normal rate pnd = w x n, capsule end-point velocities va / vb, the linear advance over the micro-steps of a substep, the bound) is
written three times for the floating-base tree (lane path, quad kernel, chain-wave kernel).  tests/ta_branch_scenarios.py reaches the paddle with
a humanoid standing at rest, where every one of those terms is zero and substep 0 and substep 1 see the same geometry.

`scenarios`: every env is a humanoid in a drawn pose inside the limits with a displaced, rotated root.  In half the envs of every group the joint
rates and the root's linear / angular velocity are drawn and so are the actions; the other half starts at rest, its legs in the standing pose and
the actions holding the drawn pose.  The group is GROUP_CYCLE[env % 19] (paddle, the six shapes, broad phase, scene bodies); inside a group the
sub-case, at rest / moving and the substep aimed at cycle with the env's index.  The ball is AIMED (ball_contact_scenarios.launch: the oracle's
free flight backwards) at where a first oracle pass with the ball parked far away finds the target link at the start of the aimed SUBSTEP of step
(env % 7) % 3 of STEPS — the oracle with substeps = 1 and dt / 2 is the oracle's first substep, so both substeps' start geometry are oracle tensors.

Everything is decided from the ORACLE and the config, never from a kernel's output:
  * CLASS (which body): the main oracle's ball differs by more than REACHED = 100 x the comparison tolerance from that of a counterfactual oracle
    stepped from the same state whose Config has that body taken away (ball_contact_scenarios.counterfactual_configs).
  * SUB-CASE: fp64 geometry of this module on the oracle's pre-step tensors and its tensors after the first substep: the ball flies freely to the
    first micro-step at which a body's separation is below contact_offset; in a substep the bodies move linearly from their pose at its start; an
    env-step counts only where that body is the only one active there.
  * MOVING: the contact point moves at >= MOVING_SPEED, AND the oracle stepped from the same pose with the velocities that move that body's link
    (the root's twist and the joint rates between the root and the link) zeroed in the INPUT STATE differs from the main run by REACHED x the
    tolerance: a different state, the same code.  A substep-1 cell further needs the contact point (fixed in its link) to have travelled at least
    TRAVEL = 20 x TOL["rb_pos"] = 2 mm during substep 0.  So a kernel that drops a point's velocity, or a ball wave that reads the other substep's
    hand-off slot, cannot agree with the oracle in those cells.
  * AT REST: an env that started the scenario at rest, the contact point slower than REST_SPEED (what gravity and the holding drive give it in a
    step or two); the old comparison, and what the moving cells differ from.
  * The broad-phase cells are geometry alone, and there the oracle without the whole humanoid must agree with the main run exactly."""
import functools

import numpy as np

import ta_branch_scenarios as tb
from ball_contact_scenarios import (EDGE_FACTOR, REACHED, SHAPES, _box, _capsule, _disc, _dot, _micro, _mv, _quat_rot, _resolve_terms, _unit,
                                    counterfactual_configs, launch)
from isaacgym_amd import scene

STEPS = 3
FLOOR = 8                    # kept env-steps every cell must reach
ENV_SEED = tb.ENV_SEED
EXCLUDED_BOUND = tb.EXCLUDED_BOUND
MOVING_SPEED = 0.5           # m/s of the contact point: a "moving" cell
REST_SPEED = 0.1             # m/s: an "at rest" cell (an env that STARTED at rest; the drive and gravity move it a little within the three steps)
TRAVEL_FACTOR = 20.0         # x TOL["rb_pos"]: what the contact point must have travelled during substep 0 for a substep-1 cell
BODY_LINK = dict(paddle=27, hand=27, forearm=24, upper_arm=24, torso=15, pelvis=0, head=15)
CAPSULES, SPHERES = ("forearm", "upper_arm", "torso"), ("hand", "pelvis", "head")
MOTION = ("rest", "moving/sub0", "moving/sub1")

CELLS = ([f"paddle/{k}/{mo}/{su}" for k in ("front", "back", "rim", "inside") for mo in ("rest", "moving") for su in ("sub0", "sub1")] +
         [f"shape/{s}/{mo}" for s in SPHERES for mo in MOTION] +
         [f"capsule/{s}/{w}/{mo}" for s in CAPSULES for w in ("interior", "end0", "end1") for mo in MOTION] +
         ["broad/inside_bound", "broad/outside_bound"] +
         ["scene/ground", "scene/net_face_pos_x", "scene/net_face_neg_x", "scene/table_long_edge", "scene/table_underside"])
NO_EFFECT = ("broad/inside_bound", "broad/outside_bound")
MOVING_CELLS = tuple(c for c in CELLS if "/moving" in c)
SUB1_CELLS = tuple(c for c in CELLS if c.endswith("sub1"))
EDGE_CELLS = tuple(c for c in CELLS if "/rim/" in c or "/end0/" in c or "/end1/" in c or c == "scene/table_long_edge")

# group of env e: GROUP_CYCLE[e % 19] — 0 paddle (16 cells), 1 hand, 2 forearm, 3 upper arm, 4 torso (9 cells each), 5 pelvis, 6 head, 7 broad phase,
# 8 scene bodies.  19 shares no factor with the 7 and the 3 of the step rule.
GROUP_CYCLE = (0, 2, 3, 4, 0, 1, 2, 5, 0, 3, 4, 6, 0, 2, 7, 3, 0, 4, 8)
GROUP_BODY = ("paddle", "hand", "forearm", "upper_arm", "torso", "pelvis", "head")
KINDS = {0: 4, 1: 1, 2: 3, 3: 3, 4: 3, 5: 1, 6: 1, 7: 2, 8: 5}


def groups_of(n):
    """-> (group [n], case [n]: the running index of the env inside its group)."""
    cycle = np.array(GROUP_CYCLE)
    G, env = len(cycle), np.arange(n)
    rank = np.array([int((cycle[:i] == cycle[i]).sum()) for i in range(G)])
    mult = np.array([int((cycle == g).sum()) for g in cycle])
    return cycle[env % G], (env // G) * mult[env % G] + rank[env % G]


def half_config(cfg):
    """The oracle's first substep as a step of its own: substeps = 1, dt / 2 (h = dt / substeps and hb = h / ball_substeps are unchanged)."""
    c = scene.Config.from_buffer_copy(cfg)
    assert cfg.substeps == 2
    c.substeps, c.dt = 1, cfg.dt / 2
    return c


def ancestors(m, link):
    """The dofs (joint of link i = dof i - 1) between the root and `link`."""
    out = []
    while link > 0:
        out.append(link - 1)
        link = m.link[link].parent
    return out


class Humanoid:
    """World geometry of the paddle, the shapes and the bound at the start of a substep, from rigid_body_states [n, 42, 13] (row link.body = pose,
    linear and angular velocity of that link's origin, world frame) and the config: the interface of ball_contact_scenarios.Arm."""

    def __init__(self, cfg, m, rb):
        rb = np.asarray(rb, np.float64)
        self.n, self.cfg = rb.shape[0], cfg
        rows = rb[:, [m.link[i].body for i in range(28)]]
        self.p, self.v, self.w = rows[:, :, 0:3], rows[:, :, 7:10], rows[:, :, 10:13]
        self.R = np.stack([_quat_rot(rows[:, j, 3:7]) for j in range(28)], axis=1)
        L = cfg.paddle_link
        self.pc, self.vpc = self.point(L, list(cfg.paddle_center))
        self.pn = _mv(self.R[:, L], np.array(list(cfg.paddle_normal), np.float64))
        self.pnd = np.cross(self.w[:, L], self.pn)
        self.bound, self.vbound = self.point(m.bound_link, list(m.bound_center))

    def point(self, link, local):
        off = _mv(self.R[:, link], np.array(local, np.float64))
        return self.p[:, link] + off, self.v[:, link] + np.cross(self.w[:, link], off)

    def shape(self, s):
        sh = self.cfg.shape[s]
        (a, va), (b, vb) = self.point(sh.link, list(sh.a)), self.point(sh.link, list(sh.b))
        return a, va, b, vb, float(sh.radius)

    def paddle_at(self, t):
        t = np.asarray(t, np.float64).reshape(-1, 1) * np.ones((self.n, 1))
        return self.pc + self.vpc * t, _unit(self.pn + self.pnd * t)

    def to_local(self, link, x):
        return np.einsum("nji,nj->ni", self.R[:, link], x - self.p[:, link])

    def to_world(self, link, local):
        return self.p[:, link] + np.einsum("nij,nj->ni", self.R[:, link], local)

    def bodies(self, p, t):
        """{body: terms of ball_contact_scenarios._disc / _capsule} of ball centres p [n,3], t [n] or scalar after the substep's start."""
        t = np.asarray(t, np.float64).reshape(-1, 1) * np.ones((self.n, 1))
        C, N = self.paddle_at(t)
        out = {"paddle": _disc(self.cfg, p, C, N, self.vpc, self.pnd)}
        for s_, name in enumerate(SHAPES):
            a0, va, b0, vb, radius = self.shape(s_)
            out[name] = _capsule(self.cfg, p, a0 + va * t, b0 + vb * t, va, vb, radius)
        return out


# ------------------------------------------------------------------------------------------------------------------ the scripted states
def dr_tables(n, seed):
    """The tables of the randomised case: per-env restitution and friction scales, gains and masses left at 1 (the aimed states still land).
    restitution_scale in [1.3, 1.6] in the paddle and shape groups (0.8 x 1.3 > restitution_max = 1: the clamp binds), in (0, 0.7) elsewhere."""
    rng = np.random.default_rng([seed, 77])
    group, _ = groups_of(n)
    u = lambda lo, hi: rng.uniform(lo, hi, n).astype(np.float32)
    return dict(restitution_scale=np.where(group <= 6, u(1.3, 1.6), u(0.0, 0.7)).astype(np.float32), friction_scale=u(0.7, 1.3))


def _quat_mul(a, b):
    ax, ay, az, aw = (a[:, i] for i in range(4))
    bx, by, bz, bw = (b[:, i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=1)


def _axis_angle(axis, ang):
    return np.concatenate([_unit(axis) * np.sin(ang / 2)[:, None], np.cos(ang / 2)[:, None]], axis=1)


def scenarios(n, seed):
    """-> root [n,3,13], dof [n,27,2], progress [n] int64, actions [n,27] (held over the STEPS steps), meta (group / kind / moving / sub / when [n])."""
    from oracle import binding
    binding.build()
    p, cfg, m = scene.build_ta_params(n), scene.build_ta_scene(n), scene.build_ta_model()
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    pm = lambda: rng.choice([-1.0, 1.0], n)
    deg = np.pi / 180
    env = np.arange(n)
    (group, case), when = groups_of(n), (env % 7) % 3
    K = np.array([KINDS[g] for g in range(9)])[group]
    kind, moving, sub = case % K, (case // K) % 2 == 1, (case // (2 * K)) % 2
    per, hb = _micro(cfg)
    M = cfg.ball_substeps
    mc = sub * M + rng.integers(0, M, n)                      # the micro-step of the step aimed at: both substeps are hit
    r, off = float(cfg.ball_radius), float(cfg.contact_offset)

    # ---- the humanoid: pose inside the limits, root displaced and rotated; half the envs of every group moving, the others at rest with
    #      their legs in the standing pose (the soles flat on the ground) and the actions holding the pose
    lo, hi = (np.array([getattr(m.link[i], k) for i in range(1, 28)], np.float64) for k in ("lower", "upper"))
    q = np.array(list(p.init_dof_pos), np.float64)[None, :] + rng.uniform(-0.3, 0.3, (n, 27))
    q[~moving, 0:12] = np.array(list(p.init_dof_pos), np.float64)[0:12]
    q = np.clip(q, lo + 0.01, hi - 0.01)
    qd = rng.uniform(-4.0, 4.0, (n, 27)) * moving[:, None]
    root = np.zeros((n, 3, 13), np.float64)
    for a in range(3):
        root[:, a, :7] = np.array(list(p.init_root[a]))
    root[:, 0, 0:2] += rng.uniform(-0.1, 0.1, (n, 2))
    root[:, 0, 2] += np.where(moving, u(0.0, 0.08), 0.0)
    yaw = _axis_angle(np.tile([0.0, 0, 1.0], (n, 1)), u(-0.4, 0.4))
    tilt = _axis_angle(rng.normal(size=(n, 3)), np.where(moving, u(-0.25, 0.25), 0.0))
    root[:, 0, 3:7] = _quat_mul(_quat_mul(tilt, yaw), root[:, 0, 3:7])
    root[:, 0, 7:10] = rng.uniform(-0.8, 0.8, (n, 3)) * moving[:, None]
    root[:, 0, 10:13] = rng.uniform(-2.0, 2.0, (n, 3)) * moving[:, None]
    hold = np.clip((q - 0.5 * (hi + lo)) / (0.5 * (hi - lo)), -1.0, 1.0)
    actions = np.ascontiguousarray(np.where(moving[:, None], rng.uniform(-1.0, 1.0, (n, 27)), hold), np.float32)
    dof = np.ascontiguousarray(np.stack([q, qd], axis=2), np.float32)
    root[:, 2, 0:3] = np.array([10.0, 10.0, 5.0])             # first pass: the ball parked far away
    root = root.astype(np.float32)

    half = half_config(cfg)
    r1, d1 = root.copy(), dof.copy()
    rbs = np.zeros((STEPS, 2, n, 42, 13))
    for t in range(STEPS):
        rbs[t, 0] = binding.ta_forward_kinematics(m, r1, d1)
        r2, d2 = r1.copy(), d1.copy()
        rbs[t, 1] = binding.ta_simulate(half, m, actions, r2, d2, threads=8)[0]
        binding.ta_simulate(cfg, m, actions, r1, d1, threads=8)
    H = Humanoid(cfg, m, rbs[when, sub, env])
    tc = (mc % M) * hb

    P, V = np.zeros((n, 3)), np.zeros((n, 3))
    W = rng.uniform(-30, 30, (n, 3))
    vn = u(1.5, 5.0)                                          # approach speed along the normal, relative to the body
    s = off - u(0.15, 0.85) * vn * hb                         # separation at the activating micro-step: outside the zone one micro-step earlier

    def tangent(d, lo_, hi_):
        return _unit(np.cross(d, _unit(rng.normal(size=(n, 3))))) * u(lo_, hi_)[:, None]

    def clearance(pos, but):
        """Smallest separation of a ball at `pos` from the humanoid's bodies other than `but`."""
        return np.min([b["s"] for k, b in H.bodies(pos, tc).items() if k != but], axis=0)

    def best(candidates, but):
        """Of the candidate (position, velocity) pairs, per env the one farthest from every other body."""
        clear = np.stack([clearance(c[0], but) for c in candidates])
        pick = np.argmax(clear, axis=0)
        return tuple(np.stack([c[i] for c in candidates])[pick, env] for i in range(2))

    # ---- paddle: front face, back face, rim, centre inside the blade (flown in fast enough to pass the offset zone and the face in one micro-step)
    R_, tp_ = float(cfg.paddle_radius), float(cfg.paddle_half_thickness)
    L = cfg.paddle_link
    C, N = H.paddle_at(tc)
    cands = []
    for _ in range(12):
        ang = u(-70, 70) * deg                                # in the blade's plane, on the far side from the hand
        e = _mv(H.R[:, L], np.array([1.0, 0, 0])) * np.cos(ang)[:, None] + _mv(H.R[:, L], np.array([0, 0, 1.0])) * np.sin(ang)[:, None]
        e = _unit(e - N * _dot(e, N)[:, None])
        sg = np.where(kind == 0, 1.0, np.where(kind == 1, -1.0, pm()))
        ph, rho, hh = u(15, 70) * deg, u(0.0, 0.06), u(0.0005, 0.004)
        rim, inside = (kind == 2)[:, None], (kind == 3)[:, None]
        dirn = np.where(rim, e * np.cos(ph)[:, None] + N * (sg * np.sin(ph))[:, None], N * sg[:, None])
        closest = C + np.where(rim, e * R_, e * rho[:, None]) + N * (sg * tp_)[:, None]
        surf = H.vpc + np.cross(np.cross(N, H.pnd), closest - C)
        fast = (tp_ - hh + r + off + u(0.002, 0.006)) / hb
        pos = np.where(inside, C + e * rho[:, None] + N * (sg * hh)[:, None], closest + dirn * (r + s)[:, None])
        vel = surf + np.where(inside, -N * (sg * fast)[:, None], -dirn * vn[:, None]) + np.cross(N, e) * u(-2, 2)[:, None]
        cands.append((pos, vel))
    g_ = group == 0
    pos, vel = best(cands, "paddle")
    P[g_], V[g_] = pos[g_], vel[g_]

    # ---- the six shapes: spheres from any side, capsules on their interior / end a / end b; of 16 drawn directions the one clearest of the neighbours
    for gi in range(1, 7):
        name = GROUP_BODY[gi]
        si = SHAPES.index(name)
        a0, va, b0, vb, Rs = H.shape(si)
        aw, bw = a0 + va * tc[:, None], b0 + vb * tc[:, None]
        capsule = name in CAPSULES
        axis = _unit(bw - aw) if capsule else np.tile([0.0, 0, 1.0], (n, 1))
        cands = []
        for _ in range(16):
            rnd = _unit(rng.normal(size=(n, 3)))
            perp = _unit(rnd - axis * _dot(rnd, axis)[:, None])
            ph = u(0, 65) * deg
            cap = lambda sgn: axis * (sgn * np.cos(ph))[:, None] + perp * np.sin(ph)[:, None]
            if capsule:
                d = np.select([(kind == 0)[:, None], (kind == 1)[:, None]], [perp, cap(-1.0)], cap(1.0))
                tpar = np.select([kind == 0, kind == 1], [u(0.25, 0.75), 0.0], 1.0)
            else:
                d, tpar = rnd, np.zeros(n)
            cp = aw + (bw - aw) * tpar[:, None]
            cands.append((cp + d * (Rs + r + s)[:, None], va + (vb - va) * tpar[:, None] - d * vn[:, None] + tangent(d, 0, 1.5)))
        g_ = group == gi
        pos, vel = best(cands, name)
        P[g_], V[g_] = pos[g_], vel[g_]

    # ---- broad phase: just inside / just outside the bound, which rides on the torso of a displaced, rotated, moving root; the ball moves with it
    g_ = group == 7
    az, el = u(-60, 60) * deg, u(-10, 50) * deg
    d = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], axis=1)
    rad = float(cfg.humanoid_bound_radius) + np.where(kind == 0, -1.0, 1.0) * u(0.006, 0.03)
    P[g_], V[g_] = (H.bound + H.vbound * tc[:, None] + d * rad[:, None])[g_], (H.vbound + tangent(d, 0.3, 1.0))[g_]

    # ---- scene bodies under the 27-dof constants: ground at TA_GROUND_Z, net face +x / -x, the table's long edge and its underside (the far half)
    g_ = group == 8
    c, h = np.array(list(cfg.table.center), np.float64), np.array(list(cfg.table.half), np.float64)
    nc, nh = np.array(list(cfg.net.center), np.float64), np.array(list(cfg.net.half), np.float64)
    x, y = c[0] + u(0.15, h[0] - 0.1), c[1] + u(-1, 1) * (h[1] - 0.1)
    sy, th, ang, vt = pm(), u(25, 65) * deg, u(0, 2 * np.pi), u(0.0, 1.5)
    sx = np.where(kind == 1, 1.0, -1.0)
    edge = np.stack([0 * th, sy * np.cos(th), np.sin(th)], axis=1)
    flat = np.stack([vt * np.cos(ang), vt * np.sin(ang), 0 * vt], axis=1)
    z_net = u(nc[2] - nh[2] + 0.035, nc[2] + nh[2] - 0.02)    # over the table top by more than the ball's radius, under the net's top edge
    pos = [np.stack([x, y, float(cfg.ground_z) + r + s], 1),
           np.stack([nc[0] + sx * (nh[0] + r + s), y, z_net], 1), np.stack([nc[0] + sx * (nh[0] + r + s), y, z_net], 1),
           np.stack([x, c[1] + sy * h[1], c[2] + h[2] + 0 * x], 1) + edge * (r + s)[:, None], np.stack([x, y, c[2] - h[2] - r - s], 1)]
    into = np.stack([-sx * vn, u(-1, 1), u(-0.5, 0.5)], 1)
    vel = [np.stack([u(-2, 2), u(-0.3, 0.3), -vn], 1), into, into, -edge * vn[:, None] + np.stack([u(-1, 1), 0 * x, 0 * x], 1),
           flat + np.stack([0 * vn, 0 * vn, vn], 1)]
    for k in range(5):
        P[g_ & (kind == k)], V[g_ & (kind == k)] = pos[k][g_ & (kind == k)], vel[k][g_ & (kind == k)]

    p0, v0 = launch(cfg, P, V, when * per + mc)
    root[:, 2, 0:3], root[:, 2, 7:10], root[:, 2, 10:13] = p0, v0, W
    progress = rng.integers(0, p.max_episode_length - 1 - STEPS, n).astype(np.int64)      # nobody times out inside the run
    return root, dof, progress, actions, dict(group=group, kind=kind, moving=moving, sub=sub, when=when)


# ------------------------------------------------------------------------------------------------------------------ fp64 geometry of the sub-cases
def first_contact(cfg, ball, geoms):
    """Free flight of the ball [n, 13] from the pre-step state to the first micro-step at which a body's separation is below contact_offset;
    geoms[s]: the Humanoid at the start of substep s.  -> ({body: its terms there (+ active, sole, sub, micro, closest)}, found [n],
    inside the bound at every micro-step [n], outside it at every micro-step [n], smallest |distance to the bound's surface| [n])."""
    per, hb = _micro(cfg)
    M, n = cfg.ball_substeps, ball.shape[0]
    p, v, w = (np.array(ball[:, cols], np.float64) for cols in (slice(0, 3), slice(7, 10), slice(10, 13)))
    r = float(cfg.ball_radius)
    damp = max(1.0 - float(cfg.ball_angular_damping) * hb, 0.0)
    found, rec = np.zeros(n, bool), {}
    always_in, always_out, margin = np.ones(n, bool), np.ones(n, bool), np.full(n, np.inf)
    for m_ in range(per):
        H, t = geoms[m_ // M], (m_ % M) * hb
        v[:, 2] += float(cfg.gravity_z) * hb
        w = w * damp
        bodies = {"ground": dict(s=p[:, 2] - float(cfg.ground_z) - r, n=np.tile([0.0, 0, 1.0], (n, 1)), u=np.zeros((n, 3))),
                  "table": _box(cfg, cfg.table, p), "net": _box(cfg, cfg.net, p)}
        dist = np.linalg.norm(p - H.bound, axis=1)
        near = dist < float(cfg.humanoid_bound_radius)
        always_in, always_out = always_in & near, always_out & ~near
        margin = np.minimum(margin, np.abs(dist - float(cfg.humanoid_bound_radius)))
        for k, b in H.bodies(p, t).items():
            b["s"] = np.where(near, b["s"], np.inf)
            bodies[k] = b
        active = {k: b["s"] < float(cfg.contact_offset) for k, b in bodies.items()}
        count = np.sum(list(active.values()), axis=0)
        newly = ~found & (count > 0)
        for k, b in bodies.items():
            b["vrel"], b["vn"], b["vt"] = _resolve_terms(cfg, v, w, b["n"], b["u"])
            b["active"], b["sole"] = active[k] & newly, active[k] & newly & (count == 1)
            b["coord"], b["micro"], b["sub"] = np.abs(p).max(axis=1), np.full(n, m_), np.full(n, m_ // M)
            b["closest"] = p - b["n"] * (np.where(np.isfinite(b["s"]), b["s"], 0.0) + r)[:, None]     # on the blade; on a capsule's surface
            b["speed"] = np.linalg.norm(b["u"], axis=1)
            if k not in rec:
                rec[k] = {kk: np.array(vv) for kk, vv in b.items()}
            else:
                for kk, vv in b.items():
                    rec[k][kk] = np.where(newly.reshape((n,) + (1,) * (np.ndim(vv) - 1)), vv, rec[k][kk])
        found |= newly
        p = p + v * hb
    for k in rec:
        rec[k]["active"], rec[k]["sole"] = rec[k]["active"] & found, rec[k]["sole"] & found
    return rec, found, always_in, always_out, margin


def classify(cfg, ball0, geoms, reached, veldep, started_at_rest, travel_min):
    """-> ({cell: bool [n]}, edge tolerance [n], {body: (speed of the contact point, its travel during substep 0, the substep) [n]}) of one env-step.
    ball0 [n, 13]: the oracle's ball at the step's start; geoms: the Humanoid at the start of either substep (oracle tensors); reached[body]: the
    counterfactual oracle without it differs by more than REACHED x the tolerance; veldep[link]: the oracle from the state with that link's
    velocities zeroed differs by more than REACHED x the tolerance."""
    rec, found, always_in, always_out, margin = first_contact(cfg, ball0, geoms)
    n, r = ball0.shape[0], float(cfg.ball_radius)
    c, travel, info = {}, {}, {}
    edge = np.zeros(n)

    def motion(body):
        """rest / moving-in-substep-0 / moving-in-substep-1 [n] of a contact with `body`."""
        b, link = rec[body], BODY_LINK[body]
        local = geoms[1].to_local(link, b["closest"])          # the contact point, fixed in its link: where it was at the start of substep 0
        travel[body] = np.linalg.norm(geoms[1].to_world(link, local) - geoms[0].to_world(link, local), axis=1)
        info[body] = (b["speed"], travel[body], b["sub"])
        rest = started_at_rest & (b["speed"] < REST_SPEED)
        mov = (b["speed"] >= MOVING_SPEED) & veldep[link]
        return rest, mov & (b["sub"] == 0), mov & (b["sub"] == 1) & (travel[body] >= travel_min)

    def edge_tol(b, lever):
        return EDGE_FACTOR * 2.0 ** -23 * b["coord"] / lever * np.linalg.norm(b["vrel"], axis=1)

    d = rec["paddle"]
    hit = d["sole"] & reached["paddle"]
    rest, m0, m1 = motion("paddle")
    flat = hit & ~d["inside"] & ~d["rim"]
    for name, mask in (("front", flat & (d["sg"] > 0)), ("back", flat & (d["sg"] < 0)), ("rim", hit & ~d["inside"] & d["rim"]), ("inside", hit & d["inside"])):
        for su in (0, 1):
            c[f"paddle/{name}/rest/sub{su}"] = mask & rest & (d["sub"] == su)
        c[f"paddle/{name}/moving/sub0"], c[f"paddle/{name}/moving/sub1"] = mask & m0, mask & m1
        if name == "rim":                                     # the normal is (centre - closest point) / r
            edge = np.where(mask, np.maximum(edge, edge_tol(d, r)), edge)
    for s_, body in enumerate(SHAPES):
        b = rec[body]
        hit = b["sole"] & reached[body] & ~b["degenerate"]
        motions = dict(zip(MOTION, motion(body)))
        if body in SPHERES:
            assert b["sphere"].all()
            for mo, mm in motions.items():
                c[f"shape/{body}/{mo}"] = hit & mm
        else:
            assert not b["sphere"].any()
            for w, mask in (("interior", hit & (b["t"] > 0) & (b["t"] < 1)), ("end0", hit & (b["t"] == 0)), ("end1", hit & (b["t"] == 1))):
                for mo, mm in motions.items():
                    c[f"capsule/{body}/{w}/{mo}"] = mask & mm
                if w != "interior":                           # the normal is (centre - end point) / (radius + r)
                    edge = np.where(mask, np.maximum(edge, edge_tol(b, float(cfg.shape[s_].radius) + r)), edge)
    c["broad/inside_bound"] = ~found & always_in & (margin < 0.05)        # geometry alone: the host test asserts free flight there
    c["broad/outside_bound"] = ~found & always_out & (margin < 0.05)
    g = rec["ground"]
    c["scene/ground"] = g["sole"] & reached["ground"] & (g["vn"] < 0)
    k = rec["net"]
    face = k["sole"] & reached["net"] & ~k["inside"] & (k["outside_axes"] == 1) & (k["face_axis"] == 0)
    c["scene/net_face_pos_x"], c["scene/net_face_neg_x"] = face & (k["face_sign"] > 0), face & (k["face_sign"] < 0)
    t = rec["table"]
    hit = t["sole"] & reached["table"] & ~t["inside"]
    c["scene/table_long_edge"] = hit & (t["outside_axes"] == 2) & (np.abs(t["n"][:, 0]) == 0)
    c["scene/table_underside"] = hit & (t["outside_axes"] == 1) & (t["face_axis"] == 2) & (t["face_sign"] < 0)
    edge = np.where(c["scene/table_long_edge"], np.maximum(edge, edge_tol(t, r)), edge)
    assert sorted(c) == sorted(CELLS)
    return c, edge, info


# ------------------------------------------------------------------------------------------------------------------ the reference trajectory
def ball_differs(a, b, factor):
    """bool [n]: the balls of two oracle results (root [n,3,13]) differ by more than factor x the comparison tolerance (factor 0: at all)."""
    import test_ta_physics as tp
    x, y = a[:, 2].astype(np.float64), b[:, 2].astype(np.float64)
    bad = (np.abs(x[:, 0:3] - y[:, 0:3]) > factor * (tp.TOL["root_pos"] + 1e-4 * np.abs(y[:, 0:3]))).any(axis=1)
    return bad | (np.abs(x[:, 7:13] - y[:, 7:13]) > factor * (tp.TOL["root_vel"] + 1e-4 * np.abs(y[:, 7:13]))).any(axis=1)


def simulator(binding, cfg, m, tables, seed, env_id_offset, episode, progress):
    """simulate(act, root, dof) -> (rb, frc, pvx), root / dof stepped in place: the oracle's rigid-body step, through ta_simulate_dr with the tables
    (per env id: every row is stepped) where there are any."""
    if tables is None:
        return lambda act, root, dof: binding.ta_simulate(cfg, m, act, root, dof, threads=8)
    return lambda act, root, dof: binding.ta_simulate_dr(cfg, m, act, root, dof, episode, progress, seed=seed, env_id_offset=env_id_offset, threads=8, **tables)


def switch_probe(binding, cfg, m, sim, s, seed):
    """test_ta_physics.ball_switch_probe with dof_after (the bodies move fast); with tables, the same two jittered runs through ta_simulate_dr."""
    import test_ta_physics as tp
    root, dof = s["after_sim"][0], s["after_sim"][1]
    if sim is None:
        return tp.ball_switch_probe(binding, cfg, m, s["act"], s["root0"], s["dof0"], root, seed=seed, dof_after=dof)
    rng, bad = np.random.default_rng(seed), np.zeros(root.shape[0], bool)
    for _ in range(2):
        r2, d2 = tp.jittered(s["root0"], 1e-6, rng), tp.jittered(s["dof0"], 1e-6, rng)
        sim(s["act"], r2, d2)
        bad |= (np.abs(r2[:, 2, 7:10] - root[:, 2, 7:10]).max(axis=1) > 1e-3) | (np.abs(d2[..., 1] - dof[..., 1]).max(axis=1) > tp.TOL["qd"] / 3.0)
    return bad


@functools.lru_cache(maxsize=None)
def oracle_run(n, seed, dr=False, per_env_irb=False):
    """The reference trajectory of `scenarios(n, seed)`: STEPS steps of the oracle's rigid-body step + post_physics_step.  -> (params, irb, tables,
    steps); a step is ta_branch_scenarios.oracle_run's dict (root0, dof0, flags0, episode0, progress0, act, after_sim, main, switch, near, cells) plus
    edge (the rim / end-cap / edge cells' tolerance [n], 0 elsewhere), free (bool [n]: the oracle without the humanoid agrees exactly), veldep
    ({link: bool [n]}) and contact ({body: (speed, travel, substep) [n]}: classify).  Computed once per key and shared by the tests; nothing in it
    is to be written to."""
    import test_ta_physics as tp
    from oracle import binding
    binding.build()
    cfg, m, p = scene.build_ta_scene(n), scene.build_ta_model(), scene.build_ta_params(n, seed=ENV_SEED)
    root, dof, progress, act, meta = scenarios(n, seed)
    tables = dr_tables(n, seed) if dr else None
    stand = np.zeros((1, 3, 13), np.float32)
    for a in range(3):
        stand[0, a, :7] = np.array(list(p.init_root[a]))
    irb = binding.ta_forward_kinematics(m, stand, np.zeros((1, 27, 2), np.float32))       # TA:1152 initial_body_states
    p.initial_rb_shared = 0 if per_env_irb else 1
    if per_env_irb:
        irb = np.ascontiguousarray(np.broadcast_to(irb, (n, 42, 13)))
    cfs = counterfactual_configs(cfg)
    gone = scene.Config.from_buffer_copy(cfg)
    gone.humanoid_bound_radius = 1e-9
    half = half_config(cfg)
    flags, episode = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    links = sorted(set(BODY_LINK.values()))
    steps = []
    for t in range(STEPS):
        s = dict(root0=root.copy(), dof0=dof.copy(), flags0=flags.copy(), episode0=episode.copy(), progress0=progress.copy(), act=act)
        make = lambda c: simulator(binding, c, m, tables, p.seed, p.env_id_offset, s["episode0"], s["progress0"])

        def stepped(c, r0=s["root0"], d0=s["dof0"]):
            r2, d2 = r0.copy(), d0.copy()
            out = make(c)(act, r2, d2)
            return r2, d2, out
        rb, frc, pvx = make(cfg)(act, root, dof)
        s["after_sim"] = (root.copy(), dof.copy(), rb, frc, pvx)
        s["switch"] = switch_probe(binding, cfg, m, make(cfg) if dr else None, s, seed=300 + t)
        s["near"] = tb.near_threshold(s["flags0"], root, rb, irb, tp.TOL["root_pos"], tp.TOL["rb_pos"], tp.TOL["root_vel"])
        reached = {k: ball_differs(stepped(c)[0], root, REACHED) for k, c in cfs.items()}
        s["free"] = ~ball_differs(stepped(gone)[0], root, 0.0)
        s["veldep"] = {}
        for link in links:                                    # the same pose, the velocities that move this link zeroed in the input state
            r0, d0 = s["root0"].copy(), s["dof0"].copy()
            r0[:, 0, 7:13] = 0.0
            d0[:, ancestors(m, link), 1] = 0.0
            s["veldep"][link] = ball_differs(stepped(cfg, r0, d0)[0], root, REACHED)
        geoms = [Humanoid(cfg, m, binding.ta_forward_kinematics(m, s["root0"], s["dof0"])), Humanoid(cfg, m, stepped(half)[2][0])]
        s["cells"], s["edge"], s["contact"] = classify(cfg, s["root0"][:, 2], geoms, reached, s["veldep"], ~meta["moving"], TRAVEL_FACTOR * tp.TOL["rb_pos"])
        obs, rew, reset = binding.ta_post_physics_step(p, rb, irb, root, dof, frc, pvx, None, flags, episode, progress)
        s["main"] = (root.copy(), dof.copy(), rb, frc, obs, rew, reset, progress.copy(), episode.copy(), flags.copy())
        steps.append(s)
    return p, irb, tables, steps


def cell_counts(steps, kept=True):
    counts = dict.fromkeys(CELLS, 0)
    for s in steps:
        k = ~(s["switch"] | s["near"]) if kept else True
        for name, mask in s["cells"].items():
            counts[name] += int((mask & k).sum())
    return counts


def assert_floor(steps, what):
    counts, before = cell_counts(steps), cell_counts(steps, kept=False)
    for name in CELLS:
        print(f"{name:40s} {counts[name]:5d} kept of {before[name]} reached")
    low = {k: v for k, v in counts.items() if v < FLOOR}
    assert not low, f"{what}: cells under the floor of {FLOOR} kept env-steps: {low}"


def assert_excluded_share(steps, what):
    n = steps[0]["switch"].size
    aside = sum(int((s["switch"] | s["near"]).sum()) for s in steps)
    near, switch = sum(int(s["near"].sum()) for s in steps), sum(int(s["switch"].sum()) for s in steps)
    print(f"{what}: set aside {aside} of {n * STEPS} env-steps ({100 * aside / (n * STEPS):.3f} %): {near} near a threshold, {switch} on a contact switch")
    assert aside <= EXCLUDED_BOUND * n * STEPS


# ------------------------------------------------------------------------------------------------------------------ the comparison
def compare_sim(got, want, keep, edge, cfg, what, rows=slice(None)):
    """check_step on the kept env-steps: got / want = (root, dof, rb, frc) after the rigid-body step.  The env-steps in a rim / end-cap / edge cell
    carry `edge` on top, on the ball's velocity and its spin (/ (kappa r)) and on nothing else; face and interior cells keep check_step as it is."""
    import test_ta_physics as tp
    from helpers import assert_close
    face, rim = keep & (edge == 0), keep & (edge > 0)
    tp.check_step(tuple(x[face][:, rows] if i == 2 else x[face] for i, x in enumerate(got)),
                  tuple(x[face][:, rows] if i == 2 else x[face] for i, x in enumerate(want)), f"{what}, face cells")
    if not rim.any():
        return
    (root_g, dof_g, rb_g, frc_g), (root_w, dof_w, rb_w, frc_w) = (tuple(x[rim] for x in y) for y in (got, want))
    vel = np.full(root_w[..., 7:13].shape, tp.TOL["root_vel"])
    vel[:, 2, 0:3] += edge[rim][:, None]
    vel[:, 2, 3:6] += edge[rim][:, None] / (float(cfg.ball_inertia_factor) * float(cfg.ball_radius))
    tp.check_step((root_g[:, :2], dof_g, rb_g[:, :40], frc_g), (root_w[:, :2], dof_w, rb_w[:, :40], frc_w), f"{what}, edge cells")
    assert_close(root_g[:, 2, 0:3], root_w[:, 2, 0:3], f"{what}, edge cells: ball pos", atol=tp.TOL["root_pos"])
    sign = np.sign(np.sum(root_g[:, 2, 3:7] * root_w[:, 2, 3:7], axis=-1, keepdims=True))
    assert_close(root_g[:, 2, 3:7] * sign, root_w[:, 2, 3:7], f"{what}, edge cells: ball quat", atol=tp.TOL["root_quat"])
    assert_close(root_g[:, 2, 7:13], root_w[:, 2, 7:13], f"{what}, edge cells: ball vel", atol=vel[:, 2])


def compare_step(t, got, s, keep, oa, cfg, alpha):
    """test_ta_reward_branches_gpu.compare_step (run_chain_step_parity's comparisons of one step) with the edge tolerance of the rim / end-cap / edge
    cells on the ball's velocity, its spin, the ball-velocity columns 117-119 of the observation and the reward's alpha |vx|.  got = the kernel's
    (root, dof, rb, frc, obs, rew, reset, progress, episode, flags)."""
    import test_ta_physics as tp
    from helpers import assert_close
    g_root, g_dof, g_rb, g_frc, g_obs, g_rew, g_reset, g_progress, g_episode, g_flags = got
    root, dof, rb, frc, obs, rew, reset, progress, episode, flags = s["main"]
    edge = s["edge"]
    np.testing.assert_array_equal(g_reset, reset)
    np.testing.assert_array_equal(g_progress, progress)
    np.testing.assert_array_equal(g_episode, episode)
    bad = (g_flags != flags) & keep
    assert not bad.any(), (f"step {t}: flags", np.flatnonzero(bad)[:8], [hex(x) for x in g_flags[bad][:8]], [hex(x) for x in flags[bad][:8]])
    assert_close(g_rew[keep], rew[keep], f"step {t}: rew", atol=tp.TA_REW_ATOL + abs(float(alpha)) * edge[keep])
    sign = np.sign(np.sum(g_rb[..., 3:7] * rb[..., 3:7], axis=-1, keepdims=True))
    assert_close((g_rb[..., 3:7] * sign)[keep], rb[keep][..., 3:7], f"step {t}: body quat", atol=2e-4)
    compare_sim((g_root, g_dof, g_rb, g_frc), (root, dof, rb, frc), keep, edge, cfg, f"step {t}", rows=slice(0, 40))
    o_tol = np.tile(oa, (keep.sum(), 1))
    o_tol[:, 117:120] += edge[keep][:, None]
    assert_close(np.delete(g_obs, 120, axis=1)[keep], np.delete(obs, 120, axis=1)[keep], f"step {t}: obs", atol=np.delete(o_tol, 120, axis=1))
    bad = (np.abs(g_obs[:, 120].astype(np.float64) - obs[:, 120]) > tp.obs120_tol(oa, obs, obs[:, 120])) & keep
    assert not bad.any(), (f"step {t}: obs column 120", np.flatnonzero(bad)[:5], g_obs[bad, 120][:5], obs[bad, 120][:5])
