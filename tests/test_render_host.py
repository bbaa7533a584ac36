"""The ray caster without a GPU: its arithmetic (isaacgym_amd/csrc/ppenv_render_device.h, compiled by g++: render_shim_binding) against
the fp64 numpy caster of render_reference on the decided pixels, analytic cases, Scene.from_config, the camera, the ABI's refusals and
the Recorder's arithmetic and files."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import render_reference as rr
import render_shim_binding as rs
from isaacgym_amd import _lib, render, scene, urdf
from isaacgym_amd._lib import RenderCamera, RenderPosed, RenderPrim, RenderScene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "task_cfgs.json")


def bare_scene():
    sc = render.Scene("HumanoidPingpongTiltG1")
    sc.source_rows = [1, 1]
    return sc


def one_sphere(r=0.25, d=3.0):
    sc = bare_scene()
    sc.ground_z, sc.checker = -50.0, False          # a far, plain ground: the picture is the sphere and the horizon
    sc.add(render.RENDER_SPHERE, "s", (0.8, 0.3, 0.2), a=(d, 0.0, 1.0), radius=r)
    return sc, [], render.Camera((0.0, 0.0, 1.0), (d, 0.0, 1.0), fov_deg=30)


def four_kinds():
    """A capsule, a box on a rotated body row, a capped cylinder and a sphere over the checker ground, under an oblique camera."""
    sc = bare_scene()
    body = np.zeros((1, 1, 13), np.float32)
    half = 0.5 * math.radians(35.0)
    body[0, 0, :7] = [0.2, 0.6, 0.45, 0.0, 0.0, math.sin(half), math.cos(half)]
    sc.add(render.RENDER_CAPSULE, "capsule", (0.2, 0.5, 0.9), a=(-0.8, -0.5, 0.5), b=(-0.3, -0.9, 0.9), radius=0.15)
    sc.add(render.RENDER_BOX, "box", (0.2, 0.7, 0.3), source=0, row=0, a=(0.0, 0.0, 0.0), b=(0.35, 0.2, 0.45))
    sc.add(render.RENDER_CYLINDER, "cylinder", (0.8, 0.2, 0.2), a=(0.9, -0.4, 0.3), b=(1.0, -0.5, 0.75), radius=0.22)
    sc.add(render.RENDER_SPHERE, "sphere", (0.9, 0.8, 0.2), a=(-0.2, -0.2, 1.4), radius=0.2)
    return sc, [body], render.Camera((2.2, -2.6, 3.4), (0.1, -0.1, 0.4), fov_deg=40)


def _scene_case(name):
    if name == "sphere":
        return one_sphere()
    if name == "kinds":
        return four_kinds()
    return rs.task_scene(rs.TASKS[name])


@pytest.mark.parametrize("size", rs.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["sphere", "kinds", "TT", "T4", "TA"])
def test_shim_matches_the_fp64_caster_on_decided_pixels(name, size):
    sc, sources, cam = _scene_case(name)
    w, h = size
    got = rs.shim_render(sc, sources, cam, w, h)
    posed = rr.place(sc.prims, sources, 0)
    want = rr.posed_matrix(posed)
    cols = [c for c in range(20) if c != 7]
    np.testing.assert_allclose(got["posed"][0][:, cols], want[:, cols], rtol=1e-5, atol=1e-6)
    assert np.array_equal(got["posed"][0][:, 7].view(np.int32), want[:, 7].astype(np.int32))
    ref, ok = rr.decided(posed, rs.header_dict(sc), cam.eye, cam.target, cam.up, cam.fov_deg, w, h)
    dev = rs.compare(ref, ok, got["id"][0], got["rgba"][0], got["depth"][0], f"{name} {w}x{h}")
    assert np.array_equal(got["shadow"][0][ok], ref["shadow"][ok]) and np.array_equal(got["parity"][0][ok], ref["parity"][ok])
    assert len(np.unique(ref["id"])) >= 2, "the camera sees one thing only"
    print(f"{name} {w}x{h}: {100 * (1 - ok.mean()):.1f} % edge pixels, worst relative depth deviation {dev:.3g}")


def test_centre_depth_and_silhouette_area_of_a_sphere():
    r, d, w, h = 0.25, 3.0, 65, 49          # odd sizes: the centre pixel's ray is the optical axis
    sc, sources, cam = one_sphere(r, d)
    got = rs.shim_render(sc, sources, cam, w, h)
    assert got["id"][0][h // 2, w // 2] == 0
    assert abs(got["depth"][0][h // 2, w // 2] - (d - r)) <= 4e-6 * (d - r)
    # the silhouette: a cone of half angle asin(r / d) about the axis cuts the image plane in a disc of radius tan(asin(r / d)) f
    f = 0.5 * h / math.tan(math.radians(cam.fov_deg) / 2)
    rad = f * math.tan(math.asin(r / d))
    count = int((got["id"][0] == 0).sum())
    assert abs(count - math.pi * rad * rad) <= 2 * math.pi * rad, (count, math.pi * rad * rad)
    assert np.isinf(got["depth"][0][0, 0]) and got["id"][0][0, 0] == render.RENDER_ID_SKY


def test_a_point_under_a_sphere_is_in_shadow_and_its_neighbour_is_not():
    sc = bare_scene()
    sc.light = (0.0, 0.0, 1.0)
    sc.checker = False
    sc.add(render.RENDER_SPHERE, "s", (0.8, 0.3, 0.2), a=(0.0, 0.0, 1.0), radius=0.3)
    w, h, fov = 65, 49, 40.0
    for x, shadowed in ((0.0, True), (0.25, True), (0.45, False), (1.0, False)):      # the shadow of a vertical light is the disc x^2 + y^2 < 0.3^2
        cam = render.Camera((x, -4.0, 0.5), (x, 0.0, 0.0), fov_deg=fov)               # looks at the ground point (x, 0, 0) past the sphere
        got = rs.shim_render(sc, [], cam, w, h)
        assert got["id"][0][h // 2, w // 2] == render.RENDER_ID_GROUND
        assert bool(got["shadow"][0][h // 2, w // 2]) is shadowed, x
        lit = rr.rgb8(np.asarray(sc.ground_rgb[0]) * (sc.ambient + (0.0 if shadowed else sc.diffuse)))
        assert np.abs(got["rgba"][0][h // 2, w // 2, :3].astype(int) - lit).max() <= 1


def _cfgs():
    golden = json.load(open(GOLDEN))
    return [(n, golden[n]["task"] if n in golden else None) for n in sorted(scene.TASK_VARIANTS)]


@pytest.mark.parametrize("name,cfg", _cfgs(), ids=[n for n, _ in _cfgs()])
def test_scene_from_config(name, cfg):
    assert len(scene.TASK_VARIANTS) == 5
    sc = render.Scene.from_config(name, cfg)
    c = sc.config
    A = 2 if scene.TASK_VARIANTS[name] == "T4" else 1
    assert sc.table_top_z == pytest.approx(c.table.center[2] + c.table.half[2], abs=0)
    table = next(p for p in sc.prims if p["name"] == "table")
    assert table["kind"] == render.RENDER_BOX and table["a"][2] + table["b"][2] == pytest.approx(sc.table_top_z, abs=1e-7)
    robot = urdf.parse(urdf.write_g1_urdf())
    pairs = len(robot.joints)
    assert pairs == len(urdf.G1_BODY_NAMES) - 1
    bones = [p for p in sc.prims if p["kind"] == render.RENDER_BONE]
    assert len(bones) == A * pairs == len(sc.bones)
    assert sc.source_rows == [40 * A + 2, A + 2]
    for p in sc.prims:
        assert -1 <= p["row"] < sc.source_rows[p["source"]]
        if p["kind"] == render.RENDER_BONE:
            assert 0 <= p["row"] and 0 <= p["row2"] < sc.source_rows[p["source"]]
    assert len(sc.prims) <= render.RENDER_MAX_PRIMS == 160
    ball = next(p for p in sc.prims if p["name"] == "ball")
    assert (ball["source"], ball["row"], ball["radius"]) == (render.SRC_ROOT, A + 1, pytest.approx(c.ball_radius))
    shapes = [p for p in sc.prims if p["name"].startswith("shape")]
    assert len(shapes) == A * c.num_shapes and len([p for p in sc.prims if p["name"].startswith("paddle")]) == A
    paddle = next(p for p in sc.prims if p["name"] == "paddle0")
    assert paddle["row"] == urdf.G1_BODY_NAMES.index("right_wrist_yaw_link") and paddle["kind"] == render.RENDER_CYLINDER
    rb, root = sc.rest_states()
    assert rb.shape == (1, 40 * A + 2, 13) and root.shape == (1, A + 2, 13) and np.isfinite(rb).all()
    # the upload's own checks accept it (host arrays stand in for the device tensors; nothing is copied to a device: no primitives given)
    h = rs.host_header(sc, [rb, root])
    assert h.num_prims == len(sc.prims)


def test_camera_basis_is_orthonormal_and_follow_adds_x_and_y_only():
    for cam in (render.Camera((2.6, -3.1, 2.4), (0.1, 0.0, 0.5)), render.Camera((0, -3, 1), (0, 0, 1)), render.Camera((1, 2, 3), (-4, 0.5, 0.2), up=(0.1, 0, 1))):
        m = np.stack(cam.basis())
        np.testing.assert_allclose(m @ m.T, np.eye(3), atol=1e-12)
        assert np.linalg.det(m[[1, 2, 0]]) == pytest.approx(-1.0)         # right, up, -forward is right-handed
    sc = render.Scene.from_config("HumanoidPingpongTiltG1")
    cam = render.Camera.follow_root(sc)
    assert cam.follow == (render.SRC_ROOT, 0)
    eye, target = cam.eye_target((0.7, -0.4, 5.0))
    np.testing.assert_allclose(eye, [0.7, -3.4, 1.0])
    np.testing.assert_allclose(target, [0.7, -0.4, 1.0])
    with pytest.raises(ValueError):
        render.Camera((0, 0, 1), (0, 0, 1))
    with pytest.raises(ValueError):
        render.Camera((0, 0, 1), (0, 0, 2))                               # up along the view direction
    # the device's rule (render_follow, through the shim): a sphere on the followed body row stays where it is in the picture when the body
    # moves in x and y, and moves up by f * dz / distance pixels when the body moves in z (the camera does not follow z)
    sc2 = bare_scene()
    sc2.checker = False
    sc2.add(render.RENDER_SPHERE, "s", (0.8, 0.3, 0.2), source=0, row=0, radius=0.3)
    cam = render.Camera((0.0, -3.0, 1.0), (0.0, 0.0, 1.0), follow=(0, 0))
    w, h = 64, 48

    def centroid(pos):
        body = np.zeros((1, 1, 13), np.float32)
        body[0, 0, :7] = list(pos) + [0, 0, 0, 1]
        ys, xs = np.nonzero(rs.shim_render(sc2, [body], cam, w, h)["id"][0] == 0)
        return xs.mean() + 0.5, ys.mean() + 0.5
    x0, y0 = centroid((0.0, 0.0, 1.0))
    assert abs(x0 - w / 2) < 0.05 and abs(y0 - h / 2) < 0.05
    x1, y1 = centroid((0.7, -0.4, 1.0))
    assert abs(x1 - x0) < 0.05 and abs(y1 - y0) < 0.05
    x2, y2 = centroid((0.7, -0.4, 1.5))
    f = 0.5 * h / math.tan(math.radians(cam.fov_deg) / 2)
    assert abs(x2 - x0) < 0.05 and abs((y0 - y2) - f * 0.5 / 3.0) < 1.0


# ---- the ABI's refusals: code and text, from argument validation alone (no GPU, no HIP call)
def _valid():
    sc = RenderScene()
    sc.num_envs, sc.num_prims, sc.num_sources = 4, 1, 1
    sc.source[0].base, sc.source[0].env_stride, sc.source[0].row_stride, sc.source[0].rows = 0x1000, 26, 13, 2
    prims = (RenderPrim * 1)()
    prims[0].kind, prims[0].row, prims[0].radius = render.RENDER_SPHERE, 1, 0.1
    cam = RenderCamera()
    cam.eye[:], cam.target[:], cam.up[:], cam.fov_deg, cam.width, cam.height, cam.follow_row = (0, -3, 1), (0, 0, 1), (0, 0, 1), 45, 64, 48, -1
    return sc, prims, cam


P = 0x1000      # a non-NULL pointer that no refused call dereferences
EINVAL = -1


def _refused(call, text):
    L = _lib.lib()
    assert L.ppenv_gae(*[None if issubclass(t, (C.c_void_p, C._Pointer)) else 0 for t in L.ppenv_gae.argtypes]) == EINVAL       # another text first
    assert call(L) == EINVAL
    assert L.ppenv_last_error().decode() == text


def test_refusals_null_pointers():
    sc, prims, cam = _valid()
    _refused(lambda L: L.pp_render_scene_upload(None, prims, P, None), "pp_render_scene_upload: NULL pointer")
    _refused(lambda L: L.pp_render_scene_upload(C.byref(sc), None, P, None), "pp_render_scene_upload: NULL pointer")
    _refused(lambda L: L.pp_render_scene_upload(C.byref(sc), prims, None, None), "pp_render_scene_upload: NULL pointer")
    _refused(lambda L: L.pp_render_pose(C.byref(sc), P, None, 1, P, None), "pp_render_pose: NULL pointer")
    _refused(lambda L: L.pp_render_pose(C.byref(sc), P, P, 1, None, None), "pp_render_pose: NULL pointer")
    _refused(lambda L: L.pp_render_rays(C.byref(sc), C.byref(cam), P, P, 1, None, None, None, None), "pp_render_rays: NULL pointer")
    _refused(lambda L: L.pp_render_rays(C.byref(sc), None, P, P, 1, P, None, None, None), "pp_render_rays: NULL pointer")


@pytest.mark.parametrize("count", [0, -1, 17])
def test_refusals_env_count(count):
    sc, prims, cam = _valid()
    _refused(lambda L: L.pp_render_pose(C.byref(sc), P, P, count, P, None), "pp_render_pose: the env selection must have 1 .. 16 entries")
    _refused(lambda L: L.pp_render_rays(C.byref(sc), C.byref(cam), P, P, count, P, None, None, None), "pp_render_rays: the env selection must have 1 .. 16 entries")


def test_refusals_too_many_primitives():
    sc, prims, cam = _valid()
    sc.num_prims = 161
    many = (RenderPrim * 161)()
    for name, call in (("pp_render_scene_upload", lambda L: L.pp_render_scene_upload(C.byref(sc), many, P, None)),
                       ("pp_render_pose", lambda L: L.pp_render_pose(C.byref(sc), P, P, 1, P, None)),
                       ("pp_render_rays", lambda L: L.pp_render_rays(C.byref(sc), C.byref(cam), P, P, 1, P, None, None, None))):
        _refused(call, f"{name}: more than PP_RENDER_MAX_PRIMS (160) primitives, or a negative count")


@pytest.mark.parametrize("field,value", [("width", 0), ("height", -3), ("fov_deg", 0.0), ("fov_deg", 180.0)])
def test_refusals_non_positive_size(field, value):
    sc, prims, cam = _valid()
    setattr(cam, field, value)
    _refused(lambda L: L.pp_render_rays(C.byref(sc), C.byref(cam), P, P, 1, P, None, None, None),
             "pp_render_rays: width and height must be positive (at most 16384) and the field of view inside (0, 180) degrees")
    sc.num_envs = 0
    _refused(lambda L: L.pp_render_pose(C.byref(sc), P, P, 1, P, None), "pp_render_pose: num_envs must be positive and num_sources 0 .. 4")


@pytest.mark.parametrize("change", [dict(row=2), dict(row=-2), dict(source=1), dict(source=-1), dict(kind=4, row=0, row2=2), dict(kind=4, row=-1, row2=0)])
def test_refusals_primitive_source_or_row_out_of_range(change):
    sc, prims, cam = _valid()
    for k, v in change.items():
        setattr(prims[0], k, v)
    _refused(lambda L: L.pp_render_scene_upload(C.byref(sc), prims, P, None), "pp_render_scene_upload: primitive 0: source or row out of range")


def test_refusals_the_rest():
    sc, prims, cam = _valid()
    prims[0].kind = 5
    _refused(lambda L: L.pp_render_scene_upload(C.byref(sc), prims, P, None), "pp_render_scene_upload: primitive 0 has an unknown kind or a negative radius")
    sc, prims, cam = _valid()
    cam.follow_source, cam.follow_row = 0, 2
    _refused(lambda L: L.pp_render_rays(C.byref(sc), C.byref(cam), P, P, 1, P, None, None, None), "pp_render_rays: the camera's follow source or row is out of range")
    cam.follow_row = -1
    _refused(lambda L: L.pp_render_rays(C.byref(sc), C.byref(cam), P, P, 1, P + 2, None, None, None), "pp_render_rays: rgba must be 4-byte aligned")
    sc.source[0].base = None
    _refused(lambda L: L.pp_render_pose(C.byref(sc), P, P, 1, P, None), "pp_render_pose: pose source 0 has a NULL base or no rows")
    assert C.sizeof(RenderPosed) == 80 and C.sizeof(RenderPrim) == 56


# ---- Recorder
def test_ring_schedule_against_a_list_written_here():
    # (calls, length, every) -> (frames rendered, the capture() calls whose frames are kept, oldest first)
    cases = {(0, 5, 1): (0, []), (3, 5, 1): (3, [0, 1, 2]), (5, 5, 1): (5, [0, 1, 2, 3, 4]), (7, 5, 1): (7, [2, 3, 4, 5, 6]),
             (10, 3, 3): (4, [3, 6, 9]), (11, 5, 3): (4, [0, 3, 6, 9]), (1, 5, 3): (1, [0]), (20, 2, 7): (3, [7, 14]), (16, 5, 3): (6, [3, 6, 9, 12, 15])}
    for args, want in cases.items():
        assert render.ring_schedule(*args) == want, args


class _FakeRenderer:
    """Renderer's surface for a Recorder, on the CPU: frame k is filled with the value k."""

    def __init__(self, shape=(2, 4, 6, 4)):
        import torch
        self.rgba, self.device, self.k = torch.zeros(shape, dtype=torch.uint8), torch.device("cpu"), 0

    def render(self, out=None):
        out.fill_(self.k)
        self.k += 1
        return out


@pytest.mark.parametrize("calls,length,every", [(3, 5, 1), (7, 5, 1), (10, 3, 3), (16, 5, 3), (20, 2, 7), (10, 5, 2)])
def test_recorder_ring_order(calls, length, every):
    rec = render.Recorder(_FakeRenderer(), length=length, every=every)
    for _ in range(calls):
        rec.capture()
    rendered, kept = render.ring_schedule(calls, length, every)
    assert rec.captured == rendered
    frames = rec.frames()
    assert frames.shape[0] == len(kept)
    assert [int(f.flatten()[0]) for f in frames] == [k // every for k in kept]          # frame numbers in time order
    assert all((f == f.flatten()[0]).all() for f in frames)


def test_recorder_refuses_a_ring_above_2_gib_and_bad_arguments():
    with pytest.raises(ValueError, match="2 GiB"):
        render.Recorder(_FakeRenderer((16, 480, 640, 4)), length=200)
    with pytest.raises(ValueError):
        render.Recorder(_FakeRenderer(), length=0)
    with pytest.raises(ValueError):
        render.Recorder(_FakeRenderer(), every=0)


def _frames(t=4, e=2, h=6, w=8):
    f = np.zeros((t, e, h, w, 4), np.uint8)
    for k in range(t):
        f[k, 0, :, :, 0], f[k, 1, :, :, 1], f[k, :, k, k, 2] = 40 * k + 10, 200 - 30 * k, 255
    f[..., 3] = 255
    return f


def test_npy_needs_no_pil_and_tiles_the_envs_side_by_side(tmp_path):
    f = _frames()
    out = render.save_frames(f, str(tmp_path / "a.npy"))
    got = np.load(out[0])
    assert got.shape == (4, 6, 16, 3)
    assert np.array_equal(got[:, :, :8], f[:, 0, :, :, :3]) and np.array_equal(got[:, :, 8:], f[:, 1, :, :, :3])
    with pytest.raises(ValueError, match="gif"):
        render.save_frames(f, str(tmp_path / "a.mp4"))


def test_gif_round_trips_through_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    f = _frames()
    out = render.save_frames(f, str(tmp_path / "a.gif"), fps=20)
    im = Image.open(out[0])
    assert im.n_frames == 4 and im.size == (16, 6)
    im.seek(2)
    assert np.abs(np.asarray(im.convert("RGB")).astype(int) - render_tiled(f)[2]).max() <= 8          # a palette of 256 colours


def test_png_round_trips_through_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    f = _frames()
    out = render.save_frames(f, str(tmp_path / "a.png"))
    assert [os.path.basename(p) for p in out] == [f"a_{k:04d}.png" for k in range(4)]
    for k, p in enumerate(out):
        im = Image.open(p)
        assert im.size == (16, 6) and np.array_equal(np.asarray(im.convert("RGB")), render_tiled(f)[k])


def render_tiled(f):
    return np.concatenate([f[:, e, :, :, :3] for e in range(f.shape[1])], axis=2).astype(int)


def test_a_missing_pil_names_npy(tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("no PIL here")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    for ext in (".gif", ".png"):
        with pytest.raises(RuntimeError, match=r"\.npy"):
            render.save_frames(_frames(), str(tmp_path / f"a{ext}"))
    assert render.save_frames(_frames(), str(tmp_path / "b.npy"))
