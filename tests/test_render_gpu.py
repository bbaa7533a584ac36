"""The ray caster on the MI355X (isaacgym_amd.render, include/ppenv_render.h): the two kernels against their host build and the fp64
caster on the decided pixels (render_reference: the rule; render_shim_binding.DEPTH_RTOL: the bound), `posed` against a numpy composition
of the pose tensors, env selections, bitwise repeatability, rendering as a read-only observer of a stepping task, what the picture
means (the ball is where root_states says; the follow-cam keeps the root on the centre column), render() inside a captured graph, and
the Player with a Recorder.  8 envs, 64 x 48 and 72 x 40 pictures.  Need a real MI355X."""
import numpy as np
import pytest

import render_reference as rr
import render_shim_binding as rs
from test_play_gpu import checkpoint, load_policy, make_plain  # noqa: F401  (checkpoint: a fixture)

pytestmark = pytest.mark.gpu

TT, TA, T4 = rs.TASKS["TT"], rs.TASKS["TA"], rs.TASKS["T4"]
DEV = "cuda:0"
N = 8
SELECTIONS = ([0], [0, 5, 7], [3, 0, 5, 7, 7, 0, 3, 5, 0, 0, 7, 3, 5, 5, 3, 7])       # one, a few, sixteen with repeats


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def make(name, seed=4, episode_length=160):
    return make_plain(name, N, seed, episode_length=episode_length)


def random_steps(torch, task, steps, seed=11):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for _ in range(steps):
        task.step(torch.rand((task.num_envs * task.num_agents, task.num_actions), device=DEV, generator=gen) * 2 - 1)


def host_sources(r):
    return [np.ascontiguousarray(t.cpu().numpy()) for t in (r.scene.rb, r.scene.root)]


@pytest.mark.parametrize("size", rs.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", [TT, T4, TA], ids=["TT", "T4", "TA"])
def test_kernels_match_shim_and_fp64_caster(torch_cuda, name, size):
    torch = torch_cuda
    from isaacgym_amd import render
    w, h = size
    task = make(name)
    random_steps(torch, task, 12)
    decided = {}
    alone = {}
    for sel in SELECTIONS:
        r = render.Renderer(task, envs=sel, width=w, height=h, depth=True, ids=True)
        first = r.render().clone()
        torch.cuda.synchronize()
        got = dict(rgba=first.cpu().numpy(), depth=r.depth.cpu().numpy(), id=r.ids.cpu().numpy(), posed=r.posed.cpu().numpy())
        assert torch.equal(r.render(), first)                                         # the same state twice: the same bits
        sources, sc, cam = host_sources(r), r.scene, r.camera
        shim = rs.shim_render(sc, sources, cam, w, h, envs=sel)
        cols = [c for c in range(20) if c != 7]
        for k, e in enumerate(sel):
            posed = rr.place(sc.prims, sources, e)
            want = rr.posed_matrix(posed)
            np.testing.assert_allclose(got["posed"][k][:, cols], want[:, cols], rtol=1e-5, atol=1e-6, err_msg=f"posed, env {e}")
            assert np.array_equal(got["posed"][k][:, 7].view(np.int32), want[:, 7].astype(np.int32))
            if e not in decided:
                decided[e] = rr.decided(posed, rs.header_dict(sc), cam.eye, cam.target, cam.up, cam.fov_deg, w, h)
            ref, ok = decided[e]
            dev = rs.compare(ref, ok, got["id"][k], got["rgba"][k], got["depth"][k], f"kernel vs fp64, env {e}")
            assert np.array_equal(got["id"][k][ok], shim["id"][k][ok])                # ... and against the host build of the same text
            assert np.abs(got["rgba"][k].astype(int) - shim["rgba"][k].astype(int))[ok].max() <= 1
            fin = ok & np.isfinite(shim["depth"][k])
            assert np.array_equal(np.isposinf(got["depth"][k])[ok], np.isposinf(shim["depth"][k])[ok])
            assert np.all(np.abs(got["depth"][k][fin] - shim["depth"][k][fin]) <= rs.DEPTH_RTOL * shim["depth"][k][fin])
            if len(sel) == 1:
                print(f"{name} {w}x{h} env {e}: {100 * (1 - ok.mean()):.1f} % edge pixels, worst relative depth deviation from fp64 {dev:.3g}")
            alone.setdefault(e, got["rgba"][k])
            assert np.array_equal(got["rgba"][k], alone[e]), f"env {e} drawn in {sel} differs from its first picture"      # repeats and other selections: the same bits
    both = render.Renderer(task, envs=[0, 5], width=w, height=h).render().cpu().numpy()
    for k, e in enumerate((0, 5)):
        one = render.Renderer(task, envs=[e], width=w, height=h).render().cpu().numpy()
        assert np.array_equal(both[k], one[0])
    assert not np.array_equal(both[0], both[1])                                       # the envs do differ after 12 random steps


def snapshot(torch, task):
    """obs, rew, reset, progress and the env's whole state, as host arrays."""
    torch.cuda.synchronize()
    out = [t.cpu().numpy().copy() for t in (task.obs_buf, task.rew_buf, task.reset_buf, task.progress_buf)]
    if task.VARIANT == "TA":
        e = task.env
        out += [t.cpu().numpy().copy() for t in (e.root_states, e.dof_states, e.dof_force_tensor, e.pre_ball_vx, e.state.flags, e.state.episode)]
    else:
        out.append(task.env.get_state().copy())
    return out


@pytest.mark.parametrize("name", [TT, T4, TA], ids=["TT", "T4", "TA"])
def test_rendering_changes_no_env_state(torch_cuda, name):
    torch = torch_cuda
    from isaacgym_amd import render
    snaps = []
    for draw in (False, True):
        task = make(name, episode_length=12)                                           # resets happen within the 16 steps
        r = render.Renderer(task, envs=[0, 3, 7], width=64, height=48, depth=True, ids=True) if draw else None
        gen = torch.Generator(device=DEV).manual_seed(5)
        for _ in range(16):
            task.step(torch.rand((task.num_envs * task.num_agents, task.num_actions), device=DEV, generator=gen) * 2 - 1)
            if draw:
                r.render()
        snaps.append(snapshot(torch, task))
    assert len(snaps[0]) == len(snaps[1])
    for a, b in zip(*snaps):
        assert a.tobytes() == b.tobytes()


def test_the_ball_is_drawn_where_root_states_has_it(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make(TT)
    w, h = 640, 480                                                                    # the 2 cm ball is 4 pixels wide here (sub-pixel at 64 x 48)
    r = render.Renderer(task, envs=[2], width=w, height=h, ids=True)
    ball = next(i for i, p in enumerate(r.scene.prims) if p["name"] == "ball")
    for steps in (0, 5):
        random_steps(torch, task, steps)
        r.render()
        torch.cuda.synchronize()
        ys, xs = np.nonzero(r.ids.cpu().numpy()[0] == ball)
        assert len(xs) >= 4, "the ball is not in the picture"
        pos = r.scene.root.cpu().numpy()[2, r.scene.ball_row, :3].astype(np.float64)
        px, py = rr.project(pos, r.camera.eye, r.camera.target, r.camera.up, r.camera.fov_deg, w, h)
        assert abs(xs.mean() + 0.5 - px) <= 1.0 and abs(ys.mean() + 0.5 - py) <= 1.0, (steps, xs.mean() + 0.5, ys.mean() + 0.5, px, py)


def test_the_follow_cam_keeps_the_root_on_the_centre_column(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make(TA)
    w, h = 64, 48
    r = render.Renderer(task, envs=[1], width=w, height=h, depth=True, ids=True)
    ref_cam = render.Camera.follow_root(r.scene)
    # the follow rule under a camera that looks down on the humanoid (the horizontal follow-cam has the horizon, a band of grazing ground
    # hits and aliased checker cells, through the middle of so small a picture)
    cam = render.Camera((0.0, -3.0, 3.0), (0.0, 0.0, 0.6), follow=ref_cam.follow)
    r.set_camera(cam)
    moved = []
    for steps in (0, 20, 20):
        random_steps(torch, task, steps, seed=steps + 1)
        rgba = r.render().cpu().numpy()
        sources = host_sources(r)
        root = sources[1][1, 0, :3].astype(np.float64)
        moved.append(root)
        eye, target = cam.eye_target(root)                                             # x and y added, z not
        assert eye[2] == 3.0 and target[2] == 0.6
        for c in (cam, ref_cam):
            px, _ = rr.project(root, *c.eye_target(root), c.up, c.fov_deg, w, h)
            assert abs(px - w / 2) <= 1.0
        # ... and the picture IS the one of that camera: the fp64 caster under eye / target shifted by the root's x and y
        posed = rr.place(r.scene.prims, sources, 1)
        ref, ok = rr.decided(posed, rs.header_dict(r.scene), eye, target, cam.up, cam.fov_deg, w, h)
        rs.compare(ref, ok, r.ids.cpu().numpy()[0], rgba[0], r.depth.cpu().numpy()[0], f"follow-cam after {steps} steps")
    assert np.abs(moved[-1][:2] - moved[0][:2]).max() > 1e-3, "the root did not move: the test shows nothing"


@pytest.mark.parametrize("name", [TT, TA], ids=["TT", "TA"])
def test_render_replays_in_a_captured_graph(torch_cuda, name):
    """Nothing in render() reads on the host or allocates: captured once, replayed after a step, it draws the new state."""
    torch = torch_cuda
    from isaacgym_amd import render
    task = make(name)
    random_steps(torch, task, 3)
    r = render.Renderer(task, envs=[0, 6], width=72, height=40)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        r.render()                                                                     # warm-up on the capture stream
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r.render()
    before = r.rgba.clone()
    random_steps(torch, task, 4, seed=12)
    g.replay()
    torch.cuda.synchronize()
    replayed = r.rgba.clone()
    eager = r.render().clone()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, before)


def test_player_with_a_recorder(torch_cuda, checkpoint, tmp_path):  # noqa: F811
    torch = torch_cuda
    from isaacgym_amd import render
    from isaacgym_amd.play import Player
    runs = []
    for record in (False, True):
        task = make_plain(TT, N, 21)
        rec = render.Recorder(render.Renderer(task, envs=[0, 1], width=64, height=48), length=5, every=3) if record else None
        pl = Player(task, load_policy(checkpoint(TT)), games_num=4, poll_every=16, max_steps=2000, recorder=rec)
        runs.append((pl, pl.run(), rec))
    (pa, ra, _), (pb, rb, rec) = runs
    assert "captured_frames" not in ra
    strip = lambda res: {k: v for k, v in res.items() if k not in ("captured_frames", "seconds")}
    assert strip(ra) == strip(rb) and ra["games"] >= 4
    assert pa.stats.state_bytes() == pb.stats.state_bytes()
    rendered, kept = render.ring_schedule(rb["steps_played"], 5, 3)
    assert rb["captured_frames"] == rendered == (rb["steps_played"] + 2) // 3
    frames = rec.frames()
    assert tuple(frames.shape) == (len(kept), 2, 48, 64, 4) and len(kept) == 5
    assert not torch.equal(frames[0], frames[-1])
    Image = pytest.importorskip("PIL.Image")
    out = rec.save(str(tmp_path / "play.gif"), fps=30)
    im = Image.open(out[0])
    assert im.size == (128, 48) and 1 <= im.n_frames <= 5                              # PIL merges consecutive frames that are equal
    pic = pb.task.render()
    assert pic.shape == (480, 640, 3) and pic.dtype == np.uint8 and len(np.unique(pic.reshape(-1, 3), axis=0)) > 1
    assert pa.task._renderer is None                                                   # nothing but render() builds it


def test_capture_cli_writes_a_gif(torch_cuda, checkpoint, tmp_path, capsys):  # noqa: F811
    from isaacgym_amd import play
    path = str(tmp_path / "cli.gif")
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "8", "--games", "4", "--poll-every", "16", "--seed", "3", "--capture", path,
                     "--capture-envs", "0,1", "--capture-len", "4", "--capture-every", "2", "--capture-size", "72x40", "--camera", "follow"])
    out = capsys.readouterr().out
    assert res["captured_frames"] == (res["steps_played"] + 1) // 2 and "captured" in out
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(path)
    assert im.size == (144, 40) and 1 <= im.n_frames <= 4
