"""Render envs on the GPU and record a played checkpoint (C ABI: include/ppenv_render.h).

    Scene.from_config(task_name)     host only: the primitives of a task's scene from its native config and the G1 body tree
    Scene.from_task(task)            ... plus the pose tensors of a live task
    Camera.side_view(scene) / Camera.follow_root(scene)
    Renderer(task, envs=(0,), width=640, height=480, samples=1).render()     -> uint8 [E, H, W, 4] on the device, two launches, no host read
                                     samples = 2 or 4: every pixel is the box mean of samples x samples rays (pp_render_rays_aa)
    Recorder(renderer, length=100, every=1).capture() / .save("out.gif")
    TrainingCapture(renderer, out_dir, freq=1464, length=100)     gym's RecordVideo rule inside a training rollout (PPOTrainer.set_capture)
    Trajectory(renderer, length=100, every=1).capture() / .render(camera=, width=, height=, samples=) / .save("traj.npz")
                                     deferred capture: a drawn step records the POSED primitives (80 bytes each) and the camera's anchor, one
                                     small launch; all rays are cast later in one batched launch (pp_render_rays_frames), at any size, sample
                                     count and camera.  Recorder(..., deferred=True) and TrainingCapture(..., deferred=True, trajectories=True)
                                     record that way and hand out the bytes the eager recorder gives.
    Replay.load("traj.npz").render(...) / .save("out.gif")       a saved trajectory drawn again: no task, no checkpoint
    python -m isaacgym_amd.render replay traj.npz --out x.gif [--size WxH] [--samples 1|2|4] [--camera recorded|side|follow] [--fps]

WHAT IS DRAWN is the project's own UNVERIFIED collision geometry (scene.py: the capsules and spheres the ball collides with, the paddle
disc, the table slab, the net, the ball) plus a stick figure: one thin capsule ("bone") per parent-child pair of the G1 body tree
between the two bodies' origins.  No meshes, no textures; anti-aliasing is opt-in supersampling (`samples=`).  For the 7-dof tasks `rigid_body_states` carries the
pelvis and the right arm chain only (every other body row sits at the root pose), so their stick figure is the arm; the torso, pelvis
and head appear as their world-fixed collision shapes.

Rows.  `rigid_body_states` is [N, 40 * A + 2, 13] for the 7-dof tasks (A humanoids, then table and ball) and [N, 42, 13] for the
27-dof task; row 40 * h + G1_BODY_NAMES.index(name) is body `name` of humanoid h.  `root_states` is [N, A + 2, 13]: humanoids, table,
ball.  A collision shape hangs on a LINK index of the native model, mapped to its body row BY NAME:
    7-dof tasks    arm link j      -> scene.G1_RIGHT_ARM[j]["name"]  (right_shoulder_pitch_link .. right_wrist_yaw_link: rows 31 .. 37)
    27-dof task    tree link l     -> TA_LINK_NAMES[l]                (pelvis, legs, waist, left arm, the five right-arm links)
    link -1                        -> world-fixed (scene.build_config writes such shapes in world coordinates)

Out of scope: meshes, textures, mp4.
"""
import ctypes as C
import json
import math
import os

import numpy as np

from . import _lib, scene, urdf
from ._lib import (RENDER_BONE, RENDER_BOX, RENDER_CAPSULE, RENDER_CYLINDER, RENDER_ID_GROUND, RENDER_ID_SKY, RENDER_MAX_ENVS,  # noqa: F401
                   RENDER_MAX_PRIMS, RENDER_SPHERE, RenderCamera, RenderPosed, RenderPrim, RenderScene)

SRC_RB, SRC_ROOT = 0, 1                     # pp_render_scene.source[]: rigid_body_states, root_states
BONE_RADIUS = 0.02
# shading constants
LIGHT = (0.3, -0.4, 0.85)
AMBIENT, DIFFUSE = 0.35, 0.65
SKY = (0.55, 0.70, 0.90)
GROUND = ((0.55, 0.55, 0.55), (0.40, 0.40, 0.40))
CHECKER_PITCH = 1.0
COLORS = dict(bone=(0.78, 0.78, 0.82), shape=(0.25, 0.45, 0.85), shape2=(0.90, 0.55, 0.20), paddle=(0.80, 0.10, 0.10), table=(0.10, 0.35, 0.20),
              net=(0.92, 0.92, 0.92), ball=(1.00, 0.60, 0.10))
MAX_RING_BYTES = 2 << 30
POSED_WORDS = C.sizeof(RenderPosed) // 4    # 20
TRAJECTORY_VERSION = 1                      # of the .npz a Trajectory saves
# One pp_render_rays_frames launch casts at most this many rays (pixels x samples^2); cast_frames splits a recording into consecutive frame ranges.
# 20 ms at the 5.6e9 rays / s the eager kernels reach on a full MI355X (27-dof scene, 49 primitives).
MAX_LAUNCH_RAYS = 112_000_000


def _ta_link_names():
    """The 28 links of the 27-dof tree in scene.build_ta_model's order."""
    arm = [s["name"] for s in scene.G1_RIGHT_ARM]
    return (["pelvis"] + [s["name"] for s in scene._leg("left")] + [s["name"] for s in scene._leg("right")] + [s["name"] for s in scene.G1_WAIST] +
            [s["name"] for s in (scene._mirror_arm(s) for s in scene.G1_RIGHT_ARM)] + [arm[0], arm[1], arm[4], arm[5], arm[6]])


TA_LINK_NAMES = _ta_link_names()


def _rot_to_quat(r):
    """3x3 rotation -> xyzw."""
    t = np.trace(r)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = ((r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s, 0.25 * s)
    else:
        i = int(np.argmax(np.diag(r)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(1.0 + r[i, i] - r[j, j] - r[k, k]) * 2
        q = [0.0] * 4
        q[i], q[j], q[k], q[3] = 0.25 * s, (r[j, i] + r[i, j]) / s, (r[k, i] + r[i, k]) / s, (r[k, j] - r[j, k]) / s
    return np.asarray(q)


def _axis_rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)


def body_poses(robot, root_pos, root_quat, dof_pos=None):
    """Forward kinematics of the parsed body tree on the host: [40, 7] (position, quaternion xyzw) in G1_BODY_NAMES' order.
    dof_pos: {joint name: angle}, default all zero."""
    dof_pos = dof_pos or {}
    pose = {robot.root(): (np.asarray(root_pos, np.float64), scene.quat_to_rot(np.asarray(root_quat, np.float64)))}
    pending = list(robot.joints.values())
    while pending:
        rest = []
        for j in pending:
            if j.parent not in pose:
                rest.append(j)
                continue
            p, r = pose[j.parent]
            rc = r @ scene.rpy_to_rot(*j.rpy)
            if j.type != "fixed":
                rc = rc @ _axis_rot(j.axis, float(dof_pos.get(j.name, 0.0)))
            pose[j.child] = (p + r @ j.xyz, rc)
        assert len(rest) < len(pending), "the joints do not form a tree"
        pending = rest
    return np.stack([np.concatenate([pose[n][0], _rot_to_quat(pose[n][1])]) for n in urdf.G1_BODY_NAMES])


def scene_header(num_envs, num_prims, sources, c):
    """pp_render_scene: `sources` [(address, env stride, row stride, rows)] in floats; c: {name: value or array} of the header's constants."""
    h = RenderScene()
    h.num_envs, h.num_prims, h.num_sources, h.checker = int(num_envs), int(num_prims), len(sources), int(c["checker"])
    for s, (base, es, rs, rows) in zip(h.source, sources):
        s.base, s.env_stride, s.row_stride, s.rows = base, es, rs, rows
    h.ground_z, h.checker_pitch, h.ambient, h.diffuse = (float(c[k]) for k in ("ground_z", "checker_pitch", "ambient", "diffuse"))
    h.ground_rgb[0][:], h.ground_rgb[1][:] = ([float(v) for v in rgb] for rgb in c["ground_rgb"])
    h.sky_rgb[:], h.light[:] = [float(v) for v in c["sky_rgb"]], [float(v) for v in c["light"]]
    return h


class Scene:
    """The primitives of one task's scene (host data) and, after from_task, their device copy and pose sources."""

    def __init__(self, task_name):
        self.task_name = task_name
        self.variant = scene.TASK_VARIANTS[task_name]
        self.prims = []                       # dicts: kind, source, row, row2, a, b, radius, albedo, name
        self.source_rows = [0, 0]             # rows per env of rigid_body_states / root_states
        self.ground_z, self.checker, self.checker_pitch = 0.0, True, CHECKER_PITCH
        self.ground_rgb, self.sky_rgb = GROUND, SKY
        light = np.asarray(LIGHT, np.float64)
        self.light = tuple(light / np.linalg.norm(light))
        self.ambient, self.diffuse = AMBIENT, DIFFUSE
        self.header, self.prims_dev, self.sources = None, None, None

    def add(self, kind, name, albedo, source=0, row=-1, row2=-1, a=(0, 0, 0), b=(0, 0, 0), radius=0.0):
        self.prims.append(dict(kind=int(kind), name=name, source=int(source), row=int(row), row2=int(row2), a=tuple(float(v) for v in a),
                               b=tuple(float(v) for v in b), radius=float(radius), albedo=tuple(float(v) for v in albedo)))

    # ---- host
    @classmethod
    def from_config(cls, task_name, cfg=None):
        """The scene of a task by its registry name; cfg: its task cfg dict (`env`, `sim`, `scene`; default the yaml defaults).  No GPU."""
        self = cls(task_name)
        v = self.variant
        cfg = scene.default_task_cfg(v) if cfg is None else {k: (dict(x) if isinstance(x, dict) else x) for k, x in cfg.items()}
        defaults = scene.default_task_cfg(v)
        for key in ("sim", "scene"):
            cfg.setdefault(key, defaults[key])
        cfg["env"] = dict(defaults["env"], **(cfg.get("env") or {}))
        cfg["env"]["bodyStatesId"] = defaults["env"]["bodyStatesId"]          # which bodies are OBSERVED: nothing that is drawn depends on it
        table, ball = scene.asset_geometry(cfg["scene"])
        if v == "TA":
            c = scene.build_ta_scene(1, table=table, ball=ball)
            params = scene.build_ta_params(1, env={k: cfg["env"][k] for k in scene.TA_ENV_KEYS if k in cfg["env"]})
            model = scene.build_ta_model()
            link_row = [urdf.G1_BODY_NAMES.index(n) for n in TA_LINK_NAMES]
            assert link_row == [model.link[i].body for i in range(scene.TA_NUM_LINKS)], "TA_LINK_NAMES does not follow scene.build_ta_model"
            self.ground_z = float(model.ground_z)
            self._rest = dict(roots=[np.asarray(list(params.init_root[0])[:7])], table=np.asarray(list(params.init_root[1])[:7]),
                              ball=np.asarray(list(params.init_root[2])[:7]),
                              dof=dict(zip(urdf.ta_dof_joint_names(), [float(params.init_dof_pos[d]) for d in range(scene.TA_NUM_DOF)])))
        else:
            c = scene.build_config(v, cfg=cfg, num_envs=1, table=table, ball=ball)
            link_row = [urdf.G1_BODY_NAMES.index(s["name"]) for s in scene.G1_RIGHT_ARM]
            self.ground_z = float(c.ground_z)
            roots = [np.asarray(list(c.humanoid_root_pos) + list(c.humanoid_root_quat))]
            if c.num_humanoids == 2:
                roots.append(np.asarray(list(c.humanoid2_root_pos) + list(c.humanoid2_root_quat)))
            self._rest = dict(roots=roots, table=np.asarray(list(c.table_root_pos) + list(c.table_root_quat)),
                              ball=np.asarray(list(c.ball_init_pos) + list(c.ball_init_quat)), dof={})
        self.config = c
        A = self.num_humanoids = int(c.num_humanoids) if v != "TA" else 1
        nb = scene.NUM_HUMANOID_BODIES
        self.source_rows = [A * nb + 2, A + 2]
        self.robot = urdf.parse(urdf.write_g1_urdf(weld_right_elbow=(v == "TA")))
        self.table_top_z = float(c.table.center[2] + c.table.half[2])
        self.root_rows, self.ball_row = list(range(A)), A + 1

        self.add(RENDER_BOX, "table", COLORS["table"], a=list(c.table.center), b=list(c.table.half))
        self.add(RENDER_BOX, "net", COLORS["net"], a=list(c.net.center), b=list(c.net.half))
        self.add(RENDER_SPHERE, "ball", COLORS["ball"], source=SRC_ROOT, row=self.ball_row, radius=float(c.ball_radius))
        self.bones = []
        for h in range(A):
            for j in self.robot.joints.values():
                pr, ch = h * nb + urdf.G1_BODY_NAMES.index(j.parent), h * nb + urdf.G1_BODY_NAMES.index(j.child)
                self.bones.append((pr, ch))
                self.add(RENDER_BONE, f"bone{h}:{j.child}", COLORS["bone"], source=SRC_RB, row=pr, row2=ch, radius=BONE_RADIUS)
            shapes = c.shape if h == 0 else c.shape2
            for k in range(c.num_shapes):
                s = shapes[k]
                a, b = list(s.a), list(s.b)
                row = h * nb + link_row[s.link] if s.link >= 0 else -1
                self.add(RENDER_SPHERE if a == b else RENDER_CAPSULE, f"shape{h}:{k}", COLORS["shape" if h == 0 else "shape2"], source=SRC_RB, row=row,
                         a=a, b=b, radius=float(s.radius))
            pc, pn = np.asarray(list(c.paddle_center)), np.asarray(list(c.paddle_normal))
            self.add(RENDER_CYLINDER, f"paddle{h}", COLORS["paddle"], source=SRC_RB, row=h * nb + link_row[c.paddle_link],
                     a=pc - pn * c.paddle_half_thickness, b=pc + pn * c.paddle_half_thickness, radius=float(c.paddle_radius))
        if len(self.prims) > RENDER_MAX_PRIMS:
            raise ValueError(f"{len(self.prims)} primitives; the ray caster takes at most {RENDER_MAX_PRIMS}")
        return self

    def rest_states(self):
        """(rigid_body_states [1, rows, 13], root_states [1, A + 2, 13]) float32 at the task's reset pose, on the host — laid out as the
        device tensors are (for the 7-dof tasks every body row but the pelvis and the right arm chain sits at the root pose)."""
        A, nb = self.num_humanoids, scene.NUM_HUMANOID_BODIES
        rb = np.zeros((1, self.source_rows[0], 13), np.float32)
        root = np.zeros((1, self.source_rows[1], 13), np.float32)
        for h, r in enumerate(self._rest["roots"]):
            poses = body_poses(self.robot, r[:3], r[3:7], self._rest["dof"])
            if self.variant != "TA":
                keep = [0] + list(range(31, 40))
                rows = np.tile(np.concatenate([r[:3], r[3:7] / np.linalg.norm(r[3:7])]), (nb, 1))
                rows[keep] = poses[keep]
                poses = rows
            rb[0, h * nb:(h + 1) * nb, :7] = poses
            root[0, h, :7] = r
        rb[0, A * nb, :7] = root[0, A, :7] = self._rest["table"]
        rb[0, A * nb + 1, :7] = root[0, A + 1, :7] = self._rest["ball"]
        return rb, root

    def prim_array(self):
        arr = (RenderPrim * max(len(self.prims), 1))()
        for p, d in zip(arr, self.prims):
            p.kind, p.source, p.row, p.row2, p.radius = d["kind"], d["source"], d["row"], d["row2"], d["radius"]
            p.a[:], p.b[:], p.albedo[:] = d["a"], d["b"], d["albedo"]
        return arr

    def header_for(self, num_envs, sources):
        """pp_render_scene for pose tensors `sources`: [(address, env stride, row stride, rows)] in floats."""
        return scene_header(num_envs, len(self.prims), sources, vars(self))

    # ---- device
    @classmethod
    def from_task(cls, task):
        """from_config of a live task (isaacgym_amd.make) + its pose tensors + the device copy of the primitives."""
        import torch
        name = {v: k for k, v in scene.TASK_VARIANTS.items()}[task.VARIANT]
        self = cls.from_config(name, task.cfg)
        self.task, dev, n = task, task.device, task.num_envs
        self.L = task.env.L
        self.rb = torch.zeros((n, self.source_rows[0], 13), dtype=torch.float32, device=dev)      # the renderer's own: no env tensor is written
        if task.VARIANT == "TA":
            self.root = task.env.root_states                                                         # used as it is
        else:
            self.root = torch.zeros((n, self.source_rows[1], 13), dtype=torch.float32, device=dev)
        self.sources = [(t.data_ptr(), t.stride(0), t.stride(1), t.shape[1]) for t in (self.rb, self.root)]
        self.header = self.header_for(n, self.sources)
        self.prims_dev = torch.zeros(max(len(self.prims), 1) * C.sizeof(RenderPrim), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self.L.pp_render_scene_upload(C.byref(self.header), self.prim_array(), self.prims_dev.data_ptr(), _lib.stream(dev)), self.L)
            torch.cuda.current_stream(dev).synchronize()         # once: the host array must outlive the copy
        return self

    def refresh(self):
        """The pose tensors of the current state: launches only.  7-dof tasks: the gym.refresh_* kernels into the renderer's own tensors;
        27-dof task: forward kinematics of the current root / dof states (TAEnv.rb_states' kernel) into the renderer's own tensor."""
        t, s = self.task, _lib.stream(self.task.device)
        if t.VARIANT == "TA":
            t.env.sim.forward_kinematics(t.env.root_states, t.env.dof_states, self.rb)
        else:
            _lib.check(self.L.ppenv_refresh_rigid_body_states(t.env.h, self.rb.data_ptr(), s), self.L)
            _lib.check(self.L.ppenv_refresh_root_states(t.env.h, self.root.data_ptr(), s), self.L)


class Camera:
    """eye, target, up, vertical field of view.  follow: (source, row) of a body whose x and y (not z) are added to eye and target on the
    device, per env — eye and target are then offsets in x, y and absolute in z."""

    def __init__(self, eye, target, up=(0, 0, 1), fov_deg=45, follow=None):
        self.eye, self.target, self.up = (np.asarray(v, np.float64) for v in (eye, target, up))
        self.fov_deg, self.follow = float(fov_deg), follow
        f, r, u = self.basis()
        if not (np.isfinite(f).all() and np.isfinite(r).all() and 0 < self.fov_deg < 180):
            raise ValueError("Camera: eye == target, up along the view direction, or a field of view outside (0, 180)")

    def basis(self):
        """(forward, right, up) — orthonormal."""
        with np.errstate(invalid="ignore", divide="ignore"):
            f = (self.target - self.eye) / np.linalg.norm(self.target - self.eye)
            r = np.cross(f, self.up)
            r = r / np.linalg.norm(r)
        return f, r, np.cross(r, f)

    def eye_target(self, body_xyz=None):
        """What the device uses for a followed body at body_xyz: x and y added, z not."""
        if self.follow is None or body_xyz is None:
            return self.eye.copy(), self.target.copy()
        d = np.array([body_xyz[0], body_xyz[1], 0.0])
        return self.eye + d, self.target + d

    def struct(self, width, height):
        c = RenderCamera()
        c.eye[:], c.target[:], c.up[:] = self.eye, self.target, self.up
        c.fov_deg, c.width, c.height = self.fov_deg, int(width), int(height)
        c.follow_source, c.follow_row = self.follow if self.follow is not None else (0, -1)
        return c

    @classmethod
    def side_view(cls, sc, fov_deg=45):
        """The table and the humanoid(s) from the side and above, about 45 degrees down (a 4:3 picture holds them; the horizon stays out of
        the picture, where a one-sample checker would alias)."""
        c = sc.config
        xs = [r[0] for r in sc._rest["roots"]] + [c.table.center[0] - c.table.half[0], c.table.center[0] + c.table.half[0]]
        lo, hi = min(xs) - 0.6, max(xs) + 0.6
        half_h = math.tan(math.radians(fov_deg) / 2) * 4.0 / 3.0
        dist = 0.5 * (hi - lo) / half_h + c.table.half[1]
        cx = 0.5 * (lo + hi)
        return cls((cx, -0.8 * dist, 4.0), (cx, 0.0, 0.3), fov_deg=fov_deg)

    @classmethod
    def follow_root(cls, sc, fov_deg=45):
        """The reference viewer's initial follow-cam (TT:1068-1096): eye = root + (0, -3, .) at height 1.0, target = root at height 1.0."""
        return cls((0.0, -3.0, 1.0), (0.0, 0.0, 1.0), fov_deg=fov_deg, follow=(SRC_ROOT, 0))


class Renderer:
    def __init__(self, task, envs=(0,), width=640, height=480, camera=None, depth=False, ids=False, samples=1):
        import torch
        self.samples = _samples_ok("Renderer", samples)
        if self.samples > 1 and (depth or ids):
            raise ValueError("Renderer: depth and ids need samples=1: a mean of depths or ids has no meaning")
        envs = [int(e) for e in envs]
        if not 1 <= len(envs) <= RENDER_MAX_ENVS or min(envs) < 0 or max(envs) >= task.num_envs:
            raise ValueError(f"Renderer: 1 .. {RENDER_MAX_ENVS} env ids inside [0, {task.num_envs}), got {envs}")
        if int(width) < 1 or int(height) < 1:
            raise ValueError(f"Renderer: width x height must be positive, got {width} x {height}")
        self.task, self.envs, self.width, self.height = task, envs, int(width), int(height)
        self.scene = Scene.from_task(task)
        self.L, dev, E = self.scene.L, task.device, len(envs)
        self.device = dev
        self.env_ids = torch.tensor(envs, dtype=torch.int32, device=dev)
        self.posed = torch.zeros((E, max(len(self.scene.prims), 1), C.sizeof(RenderPosed) // 4), dtype=torch.float32, device=dev)
        self.rgba = torch.zeros((E, self.height, self.width, 4), dtype=torch.uint8, device=dev)
        self.depth = torch.zeros((E, self.height, self.width), dtype=torch.float32, device=dev) if depth else None
        self.ids = torch.zeros((E, self.height, self.width), dtype=torch.int32, device=dev) if ids else None
        self.set_camera(camera if camera is not None else Camera.side_view(self.scene))

    def set_camera(self, camera):
        self.camera, self._cam = camera, camera.struct(self.width, self.height)

    def render(self, out=None):
        """The selected envs as they are now -> uint8 [E, H, W, 4] on the device (`out`, default the renderer's own tensor, rewritten by
        every call; depth / ids, when asked for, land in .depth / .ids).  Launches only: nothing is read on the host, no env state changes."""
        out = self.rgba if out is None else out
        if out.dtype != self.rgba.dtype or out.shape != self.rgba.shape or not out.is_contiguous() or out.device != self.rgba.device:
            raise ValueError(f"Renderer.render: out must be a contiguous uint8 {tuple(self.rgba.shape)} tensor on {self.device}")
        sc, s = self.scene, _lib.stream(self.device)
        sc.refresh()
        _lib.check(self.L.pp_render_pose(C.byref(sc.header), sc.prims_dev.data_ptr(), self.env_ids.data_ptr(), len(self.envs), self.posed.data_ptr(), s), self.L)
        if self.samples > 1:
            _lib.check(self.L.pp_render_rays_aa(C.byref(sc.header), C.byref(self._cam), self.posed.data_ptr(), self.env_ids.data_ptr(), len(self.envs),
                                                self.samples, out.data_ptr(), s), self.L)
        else:
            _lib.check(self.L.pp_render_rays(C.byref(sc.header), C.byref(self._cam), self.posed.data_ptr(), self.env_ids.data_ptr(), len(self.envs),
                                             out.data_ptr(), _lib.ptr(self.depth), _lib.ptr(self.ids), s), self.L)
        return out


def ring_schedule(calls, length, every):
    """The Recorder's arithmetic: of `calls` capture() calls (0-based k) those with k % every == 0 render, into slot (k // every) % length.
    -> (frames rendered, [call index of each kept frame, oldest first])."""
    rendered = [k for k in range(calls) if k % every == 0]
    return len(rendered), rendered[-length:]


class _Ring:
    """The call arithmetic of Recorder and Trajectory, once (ring_schedule restates it): capture() call k (0-based) draws when k % every == 0, the
    n-th drawn call into slot n % length; the kept slots are handed out oldest first."""

    def __init__(self, who, length, every):
        if int(length) < 1 or int(every) < 1:
            raise ValueError(f"{who}: length {length} and every {every} must be positive")
        self.length, self.every = int(length), int(every)
        self.reset()

    def reset(self, base=0):                  # the next capture() is call 0, control step `base`
        self.calls, self.captured, self.base = 0, 0, int(base)

    def step(self, draw):
        """One capture() call: draw(slot) when it is a drawn one."""
        if self.calls % self.every == 0:
            draw(self.captured % self.length)
            self.captured += 1
        self.calls += 1

    def oldest_first(self, slots):
        """A tensor or a list over the slots -> its kept entries, oldest first: T = min(captured, length) of them."""
        at = self.captured % self.length
        if self.captured <= self.length:
            return slots[:self.captured]
        return slots[at:] + slots[:at] if isinstance(slots, list) else slots.roll(-at, 0) if at else slots


class Recorder:
    """The last `length` rendered frames in a device ring [length, E, H, W, 4]; capture() once per control step renders every `every`-th call.
    deferred=True: capture() records into a Trajectory (`.trajectory`; None when eager) instead of casting rays, and frames() / save() first
    cast the frames not yet drawn, batched, into the same ring slots: what a caller reads is what the eager recorder gives, byte for byte."""

    def __init__(self, renderer, length=100, every=1, deferred=False):
        import torch
        own = _Ring("Recorder", length, every)
        self.renderer, self.length, self.every = renderer, own.length, own.every
        nbytes = self.length * renderer.rgba.numel()
        if nbytes > MAX_RING_BYTES:
            raise ValueError(f"Recorder: a ring of {self.length} frames of {tuple(renderer.rgba.shape)} is {nbytes} bytes, more than "
                             f"{MAX_RING_BYTES} (2 GiB): shorten it, pick fewer envs or a smaller picture")
        self.ring = torch.zeros((self.length,) + tuple(renderer.rgba.shape), dtype=torch.uint8, device=renderer.device)
        self.trajectory = Trajectory(renderer, self.length, self.every) if deferred else None
        self._count = self.trajectory if deferred else own       # whose calls / captured these are
        self._drawn = 0                       # deferred: captured frames whose rays have been cast

    calls = property(lambda self: self._count.calls)
    captured = property(lambda self: self._count.captured)

    def reset(self, base=0):
        """Forget the frames: the next capture() is call 0 (a deferred recording numbers its steps from `base`)."""
        self._drawn = 0
        self._count.reset(base)

    def capture(self):
        if self.trajectory is not None:
            return self.trajectory.capture()
        self._count.step(lambda slot: self.renderer.render(out=self.ring[slot]))

    def flush(self):
        """Deferred: cast the rays of the captured frames not yet drawn into their ring slots (launches only; at most two slot ranges)."""
        t = self.trajectory
        if t is None or self._drawn == self.captured:
            return
        r = self.renderer
        lo = max(self._drawn, self.captured - self.length)
        a, b = lo % self.length, (self.captured - 1) % self.length + 1
        for i, j in ([(a, b)] if a < b else [(a, self.length), (0, b)]):
            cast_frames(r.L, r.scene.header, r._cam, t.posed[i:j], t.anchor[i:j], r.samples, self.ring[i:j])
        self._drawn = self.captured

    def frames(self):
        """The kept frames, oldest first: [T, E, H, W, 4] on the device, T = min(captured, length)."""
        self.flush()
        return self._count.oldest_first(self.ring)

    def save(self, path, fps=30):
        """The one host copy.  Envs side by side; *.gif (one file), *.png (numbered files <stem>_0000.png ...) through PIL, *.npy
        ([T, H, E * W, 3] uint8) without it.  -> the list of files written."""
        return save_frames(self.frames().cpu().numpy(), path, fps)


def launch_frames(samples, envs, width, height):
    """Frames one pp_render_rays_frames launch may take: at most MAX_LAUNCH_RAYS rays, 65535 frames (grid z) and fewer than 2^32 lanes; at least 1."""
    pw = 16 // samples
    lanes = -(-width // pw) * -(-height // pw) * envs * 256
    return max(1, min(MAX_LAUNCH_RAYS // (envs * width * height * samples * samples), 65535, ((1 << 32) - 1) // lanes))


def cast_frames(L, header, cam, posed, anchor, samples, out):
    """posed [T, E, P, 20] words + anchor [T, E, 4] -> out [T, E, H, W, 4] (H, W: cam's), all contiguous on one device: pp_render_rays_frames over
    consecutive frame ranges of launch_frames() frames.  Host integers and launches only."""
    T, E = int(posed.shape[0]), int(posed.shape[1])
    if tuple(out.shape) != (T, E, cam.height, cam.width, 4) or tuple(anchor.shape) != (T, E, 4) or not (posed.is_contiguous() and anchor.is_contiguous() and out.is_contiguous()):
        raise ValueError(f"cast_frames: posed {tuple(posed.shape)}, anchor {tuple(anchor.shape)} and out {tuple(out.shape)} do not belong together")
    s = _lib.stream(out.device)
    step = launch_frames(samples, E, cam.width, cam.height)
    for lo in range(0, T, step):
        n = min(step, T - lo)
        _lib.check(L.pp_render_rays_frames(C.byref(header), C.byref(cam), posed[lo].data_ptr(), anchor[lo].data_ptr(), n, E, samples, out[lo].data_ptr(), s), L)
    return out


def _frames_out(who, T, E, width, height, device):
    import torch
    nbytes = T * E * height * width * 4
    if nbytes > MAX_RING_BYTES:
        raise ValueError(f"{who}: {T} frames of {(E, height, width, 4)} are {nbytes} bytes, more than "
                         f"{MAX_RING_BYTES} (2 GiB): shorten it, pick fewer envs or a smaller picture")
    return torch.zeros((T, E, height, width, 4), dtype=torch.uint8, device=device)


def _render_frames(who, L, header, posed, anchor, given, default):
    """Trajectory.render and Replay.render: the kept frames posed [T, E, P, 20] + anchor [T, E, 4] -> a new uint8 [T, E, H, W, 4] on their device,
    under (camera, width, height, samples) = `given`, where None `default`."""
    camera, width, height, samples = (d if g is None else g for g, d in zip(given, default))
    width, height, samples = int(width), int(height), _samples_ok(who, samples)
    if width < 1 or height < 1:
        raise ValueError(f"{who}: width x height must be positive, got {width} x {height}")
    out = _frames_out(who, int(posed.shape[0]), int(posed.shape[1]), width, height, posed.device)
    return cast_frames(L, header, camera.struct(width, height), posed.contiguous(), anchor.contiguous(), samples, out) if len(out) else out


def _samples_ok(who, samples):
    if samples not in (1, 2, 4):
        raise ValueError(f"{who}: samples (sub-samples per axis) must be 1, 2 or 4, got {samples!r}")
    return int(samples)


class Trajectory(_Ring):
    """The posed primitives of the last `length` drawn control steps: a device ring posed [length, E, P, 20] (raw 32-bit words of
    pp_render_posed), anchor [length, E, 4] (x, y, z, 0 of the body a following camera follows) and, on the host, the control-step index of
    every slot.  capture() has Recorder's call arithmetic (_Ring; ring_schedule); a drawn call is scene.refresh() + pp_render_pose_anchor.
    The anchor is the renderer camera's follow body when it has one, else the first humanoid's root (SRC_ROOT, 0)."""

    def __init__(self, renderer, length=100, every=1):
        import torch
        super().__init__("Trajectory", length, every)
        self.renderer = renderer
        E, P = len(renderer.envs), max(len(renderer.scene.prims), 1)
        self.posed = torch.zeros((self.length, E, P, POSED_WORDS), dtype=torch.int32, device=renderer.device)
        self.anchor = torch.zeros((self.length, E, 4), dtype=torch.float32, device=renderer.device)
        self.steps = [0] * self.length

    def capture(self):
        self.step(self._record)

    def _record(self, slot):
        r, sc = self.renderer, self.renderer.scene
        src, row = r.camera.follow if r.camera.follow is not None else (SRC_ROOT, 0)
        sc.refresh()
        _lib.check(r.L.pp_render_pose_anchor(C.byref(sc.header), sc.prims_dev.data_ptr(), r.env_ids.data_ptr(), len(r.envs), src, row,
                                             self.posed[slot].data_ptr(), self.anchor[slot].data_ptr(), _lib.stream(r.device)), r.L)
        self.steps[slot] = self.base + self.calls

    def frames(self):
        """The kept slots, oldest first: (posed [T, E, P, 20], anchor [T, E, 4], [control-step index] * T), T = min(captured, length)."""
        return self.oldest_first(self.posed), self.oldest_first(self.anchor), self.oldest_first(self.steps)

    def render(self, camera=None, width=None, height=None, samples=None):
        """The kept frames as pictures: uint8 [T, E, H, W, 4] on the device.  The defaults are the renderer's own camera, size and sample
        count: then frame t is byte for byte what Renderer.render() drew (or would have drawn) at that step.  Launches only."""
        r = self.renderer
        return _render_frames("Trajectory.render", r.L, r.scene.header, *self.frames()[:2], (camera, width, height, samples), (r.camera, r.width, r.height, r.samples))

    def constants(self, fps=30):
        """What a file holds besides the frames (host data): the scene header's constants, the recording camera, the side view, the JSON."""
        r = self.renderer
        sc, cam, side = r.scene, r.camera, Camera.side_view(r.scene)
        f32 = lambda v: np.asarray(v, np.float32)       # noqa: E731
        meta = dict(version=TRAJECTORY_VERSION, task=sc.task_name, every=self.every, fps=float(fps), posed_words=POSED_WORDS, num_prims=len(sc.prims))
        return dict(env_ids=np.asarray(r.envs, np.int32), ground_z=f32(sc.ground_z), checker=np.asarray(int(sc.checker), np.int32),
                    checker_pitch=f32(sc.checker_pitch), ground_rgb=f32(sc.ground_rgb), sky_rgb=f32(sc.sky_rgb), light=f32(sc.light), ambient=f32(sc.ambient),
                    diffuse=f32(sc.diffuse), camera_pose=np.stack([cam.eye, cam.target, cam.up]), camera_fov=np.asarray(cam.fov_deg, np.float64),
                    camera_follow=np.asarray(int(cam.follow is not None), np.int32), camera_size=np.asarray([r.width, r.height, r.samples], np.int32),
                    side_pose=np.stack([side.eye, side.target, side.up]), side_fov=np.asarray(side.fov_deg, np.float64), meta=np.asarray(json.dumps(meta)))

    def save(self, path, fps=30):
        """One .npz, data only (write_trajectory): the one host copy.  -> path."""
        posed, anchor, steps = self.frames()
        return write_trajectory(path, posed.cpu().numpy(), anchor.cpu().numpy(), steps, self.constants(fps))


def write_trajectory(path, posed, anchor, steps, constants):
    """posed: int32 / uint32 [T, E, P, 20] on the host — stored as uint32 WORDS (the kind word is an integer: bits are kept, not values)."""
    posed = np.ascontiguousarray(posed)
    with open(path, "wb") as fh:
        np.savez(fh, posed=posed.view(np.uint32), anchor=np.asarray(anchor, np.float32), steps=np.asarray(steps, np.int64), **constants)
    return path


TRAJECTORY_KEYS = ("posed", "anchor", "steps", "env_ids", "ground_z", "checker", "checker_pitch", "ground_rgb", "sky_rgb", "light", "ambient", "diffuse",
                   "camera_pose", "camera_fov", "camera_follow", "camera_size", "side_pose", "side_fov", "meta")


def read_trajectory(path):
    """-> {key: array} of a file write_trajectory wrote, `meta` parsed.  A file that does not fit is refused by name."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in TRAJECTORY_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a trajectory file: {', '.join(missing)} missing")
        d = {k: z[k] for k in TRAJECTORY_KEYS}
    meta = d["meta"] = json.loads(str(d["meta"]))
    if meta.get("version") != TRAJECTORY_VERSION:
        raise ValueError(f"{path}: trajectory format version {meta.get('version')!r}; this build reads version {TRAJECTORY_VERSION}")
    posed = d["posed"]
    if posed.dtype != np.uint32 or posed.ndim != 4 or posed.shape[3] != POSED_WORDS or meta.get("posed_words") != POSED_WORDS:
        raise ValueError(f"{path}: {posed.shape[-1] if posed.ndim else 0} words per primitive (the file says {meta.get('posed_words')!r}); "
                         f"pp_render_posed has {POSED_WORDS}")
    num_prims = meta.get("num_prims")
    if not isinstance(num_prims, int) or not 0 <= num_prims <= RENDER_MAX_PRIMS or posed.shape[2] != max(num_prims, 1):
        raise ValueError(f"{path}: primitive count: the file says {meta.get('num_prims')!r}, its frames hold {posed.shape[2]}; the ray caster takes "
                         f"at most {RENDER_MAX_PRIMS}")
    T, E = posed.shape[:2]
    if not 1 <= E <= RENDER_MAX_ENVS or d["anchor"].shape != (T, E, 4) or d["steps"].shape != (T,) or d["env_ids"].shape != (E,):
        raise ValueError(f"{path}: {E} envs (1 .. {RENDER_MAX_ENVS}), or anchor, steps and env_ids do not match posed {posed.shape}")
    return d


class Replay:
    """A saved trajectory, drawn again without a task or a checkpoint: the arrays on `device`, the scene header rebuilt from the file's constants
    with no pose source.  A following camera (Camera(..., follow=...), any body) follows the RECORDED anchor."""

    def __init__(self, data, device="cuda:0", path=None):
        import torch
        self.data, self.meta, self.path, self.device = data, data["meta"], path, torch.device(device)
        self.posed = torch.from_numpy(np.ascontiguousarray(data["posed"]).view(np.int32)).to(self.device)
        self.anchor = torch.from_numpy(np.ascontiguousarray(data["anchor"], np.float32)).to(self.device)
        self.steps, self.envs = [int(k) for k in data["steps"]], [int(e) for e in data["env_ids"]]
        self.width, self.height, self.samples = (int(v) for v in data["camera_size"])
        self.fps = float(self.meta.get("fps", 30))
        self.header = scene_header(max(self.envs) + 1, self.meta["num_prims"], [], data)

    @classmethod
    def load(cls, path, device="cuda:0"):
        return cls(read_trajectory(path), device, path)

    def camera(self, name="recorded"):
        """recorded: the recording's own; side: Camera.side_view as the file keeps it; follow: the follow-cam on the recorded anchor."""
        d = self.data
        if name == "recorded":
            return Camera(*d["camera_pose"], fov_deg=float(d["camera_fov"]), follow=(SRC_ROOT, 0) if int(d["camera_follow"]) else None)
        if name == "side":
            return Camera(*d["side_pose"], fov_deg=float(d["side_fov"]))
        if name == "follow":
            return Camera.follow_root(None)
        raise ValueError(f"Replay.camera: {name!r} is not recorded, side or follow")

    def render(self, camera=None, width=None, height=None, samples=None):
        """uint8 [T, E, H, W, 4] on the device; the defaults are the recording's camera, size and sample count."""
        return _render_frames("Replay.render", _lib.lib(), self.header, self.posed, self.anchor, (camera, width, height, samples),
                              (self.camera(), self.width, self.height, self.samples))

    def save(self, out, fps=None, **kw):
        """render(**kw) through save_frames -> the files written."""
        return save_frames(self.render(**kw).cpu().numpy(), out, self.fps if fps is None else fps)


class TrainingCapture:
    """gym.wrappers.RecordVideo's rule (the reference's train.py:132-144: capture_video, capture_video_freq 1464, capture_video_len 100) for
    a rollout that never leaves the device: on_step(), called once after every control step, opens a recording
    <out_dir>/rl-video-step-<k><ext> at every step k with k % freq == 0 that no recording covers (k counts control steps from start_step),
    draws every `every`-th of the next `length` steps — ceil(length / every) frames, each after its step — into a device ring, and when
    the last frame is launched enqueues ONE non_blocking copy of the frames into pinned host memory and records an event.  All of that is
    host integers and launches: nothing is read from the device, so a training epoch with a recording open still has no host
    synchronisation, and the env, the policy and the learner never see it.
    poll() (main thread) hands every copy whose event has completed to the one writer thread, which touches host memory alone
    (save_frames), and returns the files finished so far; close() writes an open recording short, waits for the copies and the writer.
    The copy is ordered on the stream before any later render, so a later recording cannot overwrite frames in flight.  The pinned buffer
    allocated here serves every recording as long as each is written out before the next one ends (freq >> length: always); one more is
    allocated only when a recording ends while the writer still holds every buffer.
    deferred=True: a drawn step records into the recorder's Trajectory (refresh + one pose launch); when the recording ends the batched ray
    launch is enqueued ahead of the pinned copy — stream order keeps every guarantee above, and the files hold the same bytes.
    trajectories=True (records deferred as well): each video gets rl-video-step-<k>.traj.npz beside it, a second non_blocking copy of the posed
    words and anchors, written by the same writer thread (Replay.load draws it again at any size and camera)."""

    def __init__(self, renderer, out_dir, freq=1464, length=100, every=1, fps=30, ext=".gif", start_step=0, deferred=False, trajectories=False):
        for name, v in (("freq", freq), ("length", length), ("every", every)):
            if int(v) != v or int(v) < 1:
                raise ValueError(f"TrainingCapture: {name} {v!r} is not a positive integer")
        if int(start_step) != start_step or int(start_step) < 0:
            raise ValueError(f"TrainingCapture: start_step {start_step!r} is not a count of control steps")
        if ext not in (".gif", ".png", ".npy"):
            raise ValueError(f"TrainingCapture: ext {ext!r}: the capture formats are .gif, .png and .npy")
        if ext != ".npy":
            try:
                import PIL  # noqa: F401
            except ImportError as e:
                raise RuntimeError(f"writing {ext} needs PIL, which is not installed; pass ext='.npy' instead") from e
        self.renderer, self.out_dir, self.fps, self.ext = renderer, out_dir, fps, ext
        self.freq, self.length, self.every = int(freq), int(length), int(every)
        self.deferred, self.trajectories = bool(deferred or trajectories), bool(trajectories)
        self.recorder = Recorder(renderer, length=-(-self.length // self.every), every=self.every, deferred=self.deferred)     # one recording never wraps the ring
        self._traj_host, self._constants = {}, None     # trajectories: id(frame buffer) -> its pinned (posed, anchor); the files' constants
        self._k = int(start_step)
        self._open_at = None                  # k of the step that opened the recording in progress
        self._free = [self._host_buffer()]
        self._in_flight = []                  # [(event, path, host buffer, frames)] in stream order
        self._written, self._errors = [], []  # appended to by the writer thread (list.append: atomic), read by the main thread
        self._taken = 0                       # entries of _written the main thread has seen
        self._queue, self._thread = None, None
        self.paths = []
        os.makedirs(out_dir, exist_ok=True)

    @property
    def start_step(self):
        return self._k

    @start_step.setter
    def start_step(self, k):
        if self._open_at is not None:
            raise RuntimeError("TrainingCapture: start_step cannot change while a recording is open")
        self._k = int(k)

    @property
    def recording(self):
        return self._open_at is not None

    def _host_buffer(self):
        import torch
        pin = self.renderer.device.type == "cuda"
        host = torch.zeros(tuple(self.recorder.ring.shape), dtype=torch.uint8, pin_memory=pin)
        if self.trajectories:
            t = self.recorder.trajectory
            self._traj_host[id(host)] = (torch.zeros(tuple(t.posed.shape), dtype=t.posed.dtype, pin_memory=pin),
                                         torch.zeros(tuple(t.anchor.shape), dtype=t.anchor.dtype, pin_memory=pin))
        return host

    def on_step(self):
        """After a control step.  Host integers and launches only."""
        k = self._k
        self._k += 1
        rec = self.recorder
        if self._open_at is None:
            if k % self.freq:
                return
            self._open_at = k
            rec.reset(base=k)
        rec.capture()
        if rec.calls == self.length:
            self._finish()

    def _finish(self):
        import torch
        self._reclaim()
        rec, dev = self.recorder, self.renderer.device
        n = rec.captured
        host = self._free.pop() if self._free else self._host_buffer()
        rec.flush()                           # deferred: the batched ray launch, ahead of the copy on the stream
        host[:n].copy_(rec.ring[:n], non_blocking=True)
        traj = None
        if self.trajectories:
            t, (posed, anchor) = rec.trajectory, self._traj_host[id(host)]
            posed[:n].copy_(t.posed[:n], non_blocking=True)
            anchor[:n].copy_(t.anchor[:n], non_blocking=True)
            if self._constants is None:
                self._constants = t.constants(self.fps)
            traj = (os.path.join(self.out_dir, f"rl-video-step-{self._open_at}.traj.npz"), posed, anchor, t.steps[:n])
        event = None
        if dev.type == "cuda":
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(dev))
        self._in_flight.append((event, os.path.join(self.out_dir, f"rl-video-step-{self._open_at}{self.ext}"), host, n, traj))
        self._open_at = None

    def _reclaim(self):
        """What the writer has finished since the last look: its files, and its host buffers back to the free list."""
        while self._taken < len(self._written):
            files, host = self._written[self._taken]
            self._taken += 1
            self.paths += files
            self._free.append(host)
        if self._errors:
            raise self._errors.pop(0)

    def _write_loop(self):
        while True:
            job = self._queue.get()
            if job is None:
                return
            path, host, n, traj = job
            try:
                files = save_frames(host[:n].numpy(), path, self.fps)
                if traj is not None:
                    files = files + [write_trajectory(traj[0], traj[1][:n].numpy(), traj[2][:n].numpy(), traj[3], self._constants)]
                self._written.append((files, host))
            except Exception as e:      # noqa: BLE001  (raised on the main thread by the next poll() / close())
                self._errors.append(e)
                self._written.append(([], host))

    def _hand_over(self, wait):
        import queue
        import threading
        while self._in_flight and (wait or self._in_flight[0][0] is None or self._in_flight[0][0].query()):
            event, path, host, n, traj = self._in_flight.pop(0)
            if wait and event is not None:
                event.synchronize()
            if self._thread is None:
                self._queue = queue.Queue()
                self._thread = threading.Thread(target=self._write_loop, name="TrainingCapture writer", daemon=True)
                self._thread.start()
            self._queue.put((path, host, n, traj))

    def poll(self):
        """-> the files written so far.  Does not wait: neither for a copy nor for the writer."""
        self._hand_over(wait=False)
        self._reclaim()
        return list(self.paths)

    def close(self):
        """An open recording is written short (if it has a frame); waits for the copies and the writer.  -> all files."""
        if self._open_at is not None:
            if self.recorder.captured > 0:
                self._finish()
            self._open_at = None
        self._hand_over(wait=True)
        if self._thread is not None:
            self._queue.put(None)
            self._thread.join()
            self._thread = self._queue = None
        self._reclaim()
        return list(self.paths)


def save_frames(frames, path, fps=30):
    """frames: uint8 [T, E, H, W, 4] on the host."""
    frames = np.asarray(frames)
    T, E, H, W, _ = frames.shape
    tiled = np.ascontiguousarray(frames[..., :3].transpose(0, 2, 1, 3, 4).reshape(T, H, E * W, 3))
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        np.save(path, tiled)
        return [path]
    if ext not in (".gif", ".png"):
        raise ValueError(f"{path}: the capture formats are .gif, .png and .npy")
    if T == 0:
        raise ValueError("no frame was captured")
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"{path}: writing {ext} needs PIL, which is not installed; save to a .npy path instead") from e
    images = [Image.fromarray(f, "RGB") for f in tiled]
    if ext == ".gif":
        images[0].save(path, save_all=True, append_images=images[1:], duration=max(int(round(1000.0 / fps)), 10), loop=0)
        return [path]
    stem = os.path.splitext(path)[0]
    names = [f"{stem}_{k:04d}.png" for k in range(T)]
    for im, name in zip(images, names):
        im.save(name)
    return names


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m isaacgym_amd.render", description="draw a saved pose trajectory again (no task, no checkpoint)")
    sub = ap.add_subparsers(dest="command", required=True)
    rp = sub.add_parser("replay", help="cast the rays of a trajectory file (Trajectory.save, --capture-trajectory, --capture-trajectories)")
    rp.add_argument("trajectory", help="the .npz file")
    rp.add_argument("--out", required=True, metavar="FILE", help=".gif, .png (numbered files) or .npy")
    rp.add_argument("--size", default=None, help="WIDTHxHEIGHT of one env's picture (default: as recorded)")
    rp.add_argument("--samples", type=int, default=None, choices=(1, 2, 4), help="rays per pixel and axis (default: as recorded)")
    rp.add_argument("--camera", choices=("recorded", "side", "follow"), default="recorded", help="side: the table and humanoid(s), as the file keeps it; "
                    "follow: the follow-cam on the recorded anchor")
    rp.add_argument("--fps", type=float, default=None, help="default: as recorded")
    rp.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    width = height = None
    if args.size:
        try:
            width, height = (int(v) for v in args.size.lower().split("x"))
        except ValueError as e:
            raise SystemExit(f"--size is WIDTHxHEIGHT: {e}")
    rep = Replay.load(args.trajectory, args.device)
    files = rep.save(args.out, fps=args.fps, camera=rep.camera(args.camera), width=width, height=height, samples=args.samples)
    print(f"replayed {len(rep.steps)} frames of {rep.meta['task']}, envs {rep.envs}: {files[0]}" + (f" .. {files[-1]}" if len(files) > 1 else ""), flush=True)
    return files


if __name__ == "__main__":
    main()
