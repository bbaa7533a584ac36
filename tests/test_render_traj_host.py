"""Pose trajectories without a GPU (isaacgym_amd.render: Trajectory, Replay, write_trajectory / read_trajectory; pp_render_pose_anchor and
pp_render_rays_frames' argument checks): the file keeps every bit, a file that does not fit is refused by name, the ring arithmetic is
ring_schedule's, bad arguments are refused before any launch, the entries are bound, the CLIs list their flags."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from isaacgym_amd import _lib, play, ppo, render

TA = "HumanoidPingpongTiltNESSparse27DOFG1"
EINVAL = -1


class FakeLib:
    """Stands where the library does in a Trajectory: notes which ring slot every pose launch was pointed at."""

    def __init__(self):
        self.calls = []

    def pp_render_pose_anchor(self, header, prims, env_ids, count, source, row, posed, anchor, stream):
        self.calls.append((count, source, row, posed, anchor))
        return 0


class FakeRenderer:
    """What a Trajectory asks of a Renderer, on the host: a config-built scene, CPU tensors, no launches."""

    def __init__(self, envs=(3, 0), width=32, height=24, samples=2, camera=None):
        self.scene = sc = render.Scene.from_config(TA)
        sc.header, sc.prims_dev, sc.refresh = sc.header_for(8, []), torch.zeros(16, dtype=torch.uint8), lambda: self.refreshed.append(1)
        self.refreshed = []
        self.envs, self.width, self.height, self.samples = list(envs), width, height, samples
        self.env_ids, self.device, self.L = torch.tensor(self.envs, dtype=torch.int32), torch.device("cpu"), FakeLib()
        self.camera = camera if camera is not None else render.Camera.side_view(sc)


@pytest.fixture
def no_stream(monkeypatch):
    monkeypatch.setattr(_lib, "stream", lambda x: None)


def slots_of(traj):
    base, size = traj.posed.data_ptr(), traj.posed[0].numel() * 4
    abase, asize = traj.anchor.data_ptr(), traj.anchor[0].numel() * 4
    out = []
    for _, _, _, posed, anchor in traj.renderer.L.calls:
        assert (posed - base) % size == 0 and (posed - base) // size == (anchor - abase) // asize
        out.append((posed - base) // size)
    return out


@pytest.mark.parametrize("every", [1, 2, 3])
@pytest.mark.parametrize("length", [1, 3, 4])
def test_slot_arithmetic_is_ring_schedule(no_stream, length, every):
    for calls in (0, 1, 2, 5, 11, 12):
        r = FakeRenderer()
        traj = render.Trajectory(r, length=length, every=every)
        for _ in range(calls):
            traj.capture()
        rendered, kept = render.ring_schedule(calls, length, every)
        assert traj.calls == calls and traj.captured == rendered == len(r.L.calls) == len(r.refreshed)
        assert slots_of(traj) == [k % length for k in range(rendered)]
        posed, anchor, steps = traj.frames()
        assert steps == kept and posed.shape[0] == anchor.shape[0] == len(kept)
        traj.reset(base=100)
        traj.capture()
        assert traj.frames()[2] == [100] and slots_of(traj)[-1] == 0


def test_the_anchor_is_the_camera_s_follow_body_or_the_first_root(no_stream):
    r = FakeRenderer()
    traj = render.Trajectory(r, length=2)
    traj.capture()
    r.camera = render.Camera((0, -3, 1), (0, 0, 1), follow=(render.SRC_RB, 7))
    traj.capture()
    assert [c[:3] for c in r.L.calls] == [(2, render.SRC_ROOT, 0), (2, render.SRC_RB, 7)]
    assert tuple(traj.posed.shape) == (2, 2, len(r.scene.prims), 20) and traj.posed.dtype == torch.int32 and tuple(traj.anchor.shape) == (2, 2, 4)


def words(rng, T, E, P):
    """Random 32-bit words, the kind column among them holding integers whose float reading is a NaN, a denormal and -0."""
    w = rng.integers(0, 1 << 32, size=(T, E, P, 20), dtype=np.uint64).astype(np.uint32)
    w[..., 7] = np.asarray([0xFFFFFFFF, 0x7FC00001, 0x00000001, 0x80000000, 2], np.uint32)[rng.integers(0, 5, size=(T, E, P))]
    return w


def saved(tmp_path, no_meta=None, **over):
    r = FakeRenderer()
    traj = render.Trajectory(r, length=4)
    consts = traj.constants(fps=25)
    P = len(r.scene.prims)
    rng = np.random.default_rng(3)
    posed, anchor = words(rng, 4, 2, P), rng.standard_normal((4, 2, 4)).astype(np.float32)
    if no_meta is not None:
        meta = json.loads(str(consts["meta"]))
        meta.update(no_meta)
        consts["meta"] = np.asarray(json.dumps(meta))
    posed = over.pop("posed", posed)
    consts.update(over)
    path = render.write_trajectory(str(tmp_path / "t.traj.npz"), posed.view(np.int32), anchor, [4, 6, 8, 10], consts)
    return r, path, posed, anchor, consts


def test_the_file_keeps_every_bit(tmp_path):
    r, path, posed, anchor, consts = saved(tmp_path)
    d = render.read_trajectory(path)
    assert d["posed"].dtype == np.uint32 and d["posed"].tobytes() == posed.tobytes()
    assert d["anchor"].tobytes() == anchor.tobytes() and d["steps"].tolist() == [4, 6, 8, 10] and d["env_ids"].tolist() == [3, 0]
    for k, v in consts.items():
        if k != "meta":
            assert d[k].dtype == v.dtype and d[k].tobytes() == v.tobytes(), k
    assert d["meta"] == dict(version=1, task=TA, every=1, fps=25.0, posed_words=20, num_prims=len(r.scene.prims))
    with np.load(path, allow_pickle=False) as z:                                         # data only: nothing in it needs pickle
        assert sorted(z.files) == sorted(render.TRAJECTORY_KEYS)
    rep = render.Replay.load(path, "cpu")
    assert rep.posed.numpy().tobytes() == posed.tobytes() and rep.anchor.numpy().tobytes() == anchor.tobytes()
    assert (rep.width, rep.height, rep.samples, rep.fps, rep.envs, rep.steps) == (32, 24, 2, 25.0, [3, 0], [4, 6, 8, 10])
    h, sc = rep.header, r.scene
    want = sc.header_for(4, [])
    assert (h.num_prims, h.num_sources, h.checker) == (len(sc.prims), 0, 1)
    for f in ("ground_z", "checker_pitch", "ambient", "diffuse"):
        assert getattr(h, f) == getattr(want, f), f
    assert bytes(h.ground_rgb) == bytes(want.ground_rgb) and bytes(h.sky_rgb) == bytes(want.sky_rgb) and bytes(h.light) == bytes(want.light)
    for name, cam in (("recorded", r.camera), ("side", render.Camera.side_view(sc)), ("follow", render.Camera.follow_root(sc))):
        got = rep.camera(name)
        assert bytes(got.struct(8, 8)) == bytes(cam.struct(8, 8)), name
    with pytest.raises(ValueError, match="recorded, side or follow"):
        rep.camera("top")


def test_a_file_that_does_not_fit_is_refused_by_name(tmp_path):
    with pytest.raises(ValueError, match=r"t\.traj\.npz: trajectory format version 2; this build reads version 1"):
        render.read_trajectory(saved(tmp_path, no_meta=dict(version=2))[1])
    with pytest.raises(ValueError, match=r"t\.traj\.npz: 19 words per primitive .*pp_render_posed has 20"):
        render.read_trajectory(saved(tmp_path, posed=np.zeros((4, 2, 5, 19), np.uint32))[1])
    with pytest.raises(ValueError, match=r"t\.traj\.npz: 20 words per primitive \(the file says 24\)"):
        render.read_trajectory(saved(tmp_path, no_meta=dict(posed_words=24))[1])
    with pytest.raises(ValueError, match=r"t\.traj\.npz: primitive count: the file says 7, its frames hold"):
        render.read_trajectory(saved(tmp_path, no_meta=dict(num_prims=7))[1])
    with pytest.raises(ValueError, match=r"t\.traj\.npz: primitive count: the file says 161"):
        render.read_trajectory(saved(tmp_path, no_meta=dict(num_prims=161), posed=np.zeros((4, 2, 161, 20), np.uint32))[1])
    with pytest.raises(ValueError, match=r"t\.traj\.npz: .*do not match posed"):
        render.read_trajectory(saved(tmp_path, env_ids=np.asarray([0], np.int32))[1])
    np.savez(tmp_path / "other.npz", posed=np.zeros(3))
    with pytest.raises(ValueError, match=r"other\.npz: not a trajectory file: anchor, steps"):
        render.read_trajectory(str(tmp_path / "other.npz"))


def test_launch_frames_keeps_a_launch_under_the_ray_and_grid_limits(monkeypatch):
    monkeypatch.setattr(render, "MAX_LAUNCH_RAYS", 1 << 20)
    assert render.launch_frames(1, 1, 64, 64) == 256 and render.launch_frames(2, 1, 64, 64) == 64 and render.launch_frames(4, 16, 64, 64) == 1
    assert render.launch_frames(1, 1, 1, 1) == 65535                                       # grid z
    monkeypatch.setattr(render, "MAX_LAUNCH_RAYS", 1 << 40)
    for s, e, w, h in ((1, 1, 320, 240), (4, 16, 640, 480), (2, 3, 33, 17)):
        n = render.launch_frames(s, e, w, h)
        pw = 16 // s
        lanes = -(-w // pw) * -(-h // pw) * e * 256
        assert n * lanes < 1 << 32 and ((n + 1) * lanes >= 1 << 32 or n == 65535)
    with pytest.raises(ValueError, match=r"^Trajectory.render: 100 frames of \(16, 2048, 2048, 4\) are 26843545600 bytes, more than 2147483648 \(2 GiB\)"):
        render._frames_out("Trajectory.render", 100, 16, 2048, 2048, "cpu")


# ---- the two entries' argument checks: host-only arguments, NULL stream; validation answers before the HIP runtime is touched
def header(num_sources=2):
    sc = render.Scene.from_config(TA)
    return sc, sc.header_for(8, [(0x1000, 42 * 13, 13, 42), (0x2000, 3 * 13, 13, 3)][:num_sources])


POSE_GOOD = dict(prims=0x10, env_ids=0x20, count=2, source=1, row=0, posed=0x30, anchor=0x40)
POSE_BAD = [(dict(prims=None), "NULL pointer"), (dict(env_ids=None), "NULL pointer"), (dict(posed=None), "NULL pointer"), (dict(anchor=None), "NULL pointer"),
            (dict(count=0), "1 .. 16 entries"), (dict(count=17), "1 .. 16 entries"), (dict(row=3), "anchor's source or row"),
            (dict(source=2), "anchor's source or row"), (dict(source=-1), "anchor's source or row"), (dict(anchor=0x44), "16-byte aligned")]


@pytest.mark.parametrize("bad,text", POSE_BAD, ids=[f"{list(b)[0]}={list(b.values())[0]}" for b, _ in POSE_BAD])
def test_pose_anchor_refuses_bad_arguments_before_any_launch(bad, text):
    L = _lib.lib()
    _, h = header()
    a = dict(POSE_GOOD, **bad)
    assert L.ppenv_gae(*([None] * 2 + [0, 0] + [None] + [0, 0] + [0.0] * 3 + [None] * 3)) == EINVAL      # another text in ppenv_last_error()
    assert L.pp_render_pose_anchor(C.byref(h), a["prims"], a["env_ids"], a["count"], a["source"], a["row"], a["posed"], a["anchor"], None) == EINVAL
    msg = L.ppenv_last_error().decode()
    assert msg.startswith("pp_render_pose_anchor: ") and text in msg
    assert L.pp_render_pose_anchor(None, 0x10, 0x20, 2, 1, 0, 0x30, 0x40, None) == EINVAL


FRAMES_GOOD = dict(posed=0x100, anchor=0x200, frames=3, count=2, samples=2, rgba=0x300, width=33, height=17, follow_row=0)
FRAMES_BAD = [(dict(frames=0), "frames must be positive"), (dict(frames=-2), "frames must be positive"), (dict(count=0), "1 .. 16 entries"),
              (dict(count=17), "1 .. 16 entries"), (dict(samples=3), "1, 2 or 4"), (dict(samples=0), "1, 2 or 4"), (dict(samples=8), "1, 2 or 4"),
              (dict(posed=None), "NULL pointer"), (dict(rgba=None), "NULL pointer"), (dict(anchor=None), "needs the anchor array"),
              (dict(frames=65536, width=1, height=1), "exceed one launch's grid"), (dict(frames=100, width=16384, height=16384, samples=4), "exceed one launch's grid"),
              (dict(width=0), "width and height"), (dict(rgba=0x302), "aligned"), (dict(anchor=0x204), "aligned")]


@pytest.mark.parametrize("bad,text", FRAMES_BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b, _ in FRAMES_BAD])
def test_rays_frames_refuses_bad_arguments_before_any_launch(bad, text):
    L = _lib.lib()
    sc, h = header(num_sources=0)                                                          # a replay's header: no pose source
    a = dict(FRAMES_GOOD, **bad)
    cam = render.Camera.follow_root(sc).struct(a["width"], a["height"])
    cam.follow_row = a["follow_row"]
    assert L.ppenv_gae(*([None] * 2 + [0, 0] + [None] + [0, 0] + [0.0] * 3 + [None] * 3)) == EINVAL
    assert L.pp_render_rays_frames(C.byref(h), C.byref(cam), a["posed"], a["anchor"], a["frames"], a["count"], a["samples"], a["rgba"], None) == EINVAL
    msg = L.ppenv_last_error().decode()
    assert msg.startswith("pp_render_rays_frames: ") and text in msg
    h.num_prims = 161
    assert L.pp_render_rays_frames(C.byref(h), C.byref(cam), 0x100, 0x200, 3, 2, 2, 0x300, None) == EINVAL
    assert "num_prims" in L.ppenv_last_error().decode()


def test_the_entries_are_bound():
    L = _lib.lib()
    assert len(L.pp_render_pose_anchor.argtypes) == 9 and len(L.pp_render_rays_frames.argtypes) == 9
    assert L.pp_render_pose_anchor.argtypes[3:6] == [C.c_int32] * 3 and L.pp_render_rays_frames.argtypes[4:7] == [C.c_int32] * 3
    assert L.pp_render_rays_frames.argtypes[1] == C.POINTER(_lib.RenderCamera)


@pytest.mark.parametrize("run,flags", [(lambda: play.parse_args(["--help"]), ("--capture-deferred", "--capture-trajectory")),
                                       (lambda: ppo.main(["--help"]), ("--capture-deferred", "--capture-trajectories")),
                                       (lambda: render.main(["replay", "--help"]), ("--out", "--size", "--samples", "--camera", "--fps", "recorded"))],
                         ids=["play", "ppo", "render-replay"])
def test_help_lists_the_new_flags(capsys, run, flags):
    with pytest.raises(SystemExit) as e:
        run()
    out = capsys.readouterr().out
    assert e.value.code == 0 and all(f in out for f in flags), out
