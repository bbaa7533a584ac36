"""Pose trajectories on the MI355X (render.Trajectory / Replay / Recorder(deferred=True) / TrainingCapture(deferred=True, trajectories=True);
pp_render_pose_anchor, pp_render_rays_frames).  The yardstick for every pixel is the eager pair pp_render_pose + pp_render_rays / pp_render_rays_aa
(pinned by test_render_gpu.py and test_render_aa_gpu.py): every comparison here is torch.equal — the batched launch is the eager launches'
render_rays_kernel<S> on the same posed words (what differs is where `follow` is read and the grid's third axis), so there is no tolerance to
choose; the bytes themselves are held by test_render_digests_gpu.py.  Need a real MI355X."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from test_play_gpu import DEV, T4, TA, TT, checkpoint, load_policy, make_plain  # noqa: F401  (checkpoint: a fixture)
from test_train_capture_gpu import make_trainer, whole_state

pytestmark = pytest.mark.gpu

CONFIGS = {"TT": (TT, 64), "TA": (TA, 64), "T4": (T4, 32)}
SIZES = [(33, 17), (16, 16), (1, 1)]                                                     # ragged in both axes, one tile, one pixel
STEPS = 5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def stepper(torch, task, seed=11):
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def step():
        task.step(torch.rand((task.num_envs * task.num_agents, task.num_actions), device=DEV, generator=gen) * 2 - 1)
    return step


def selections(num_envs):
    last = num_envs - 1                                                                   # 63 with 64 envs; the 4-actor task has 32
    return [(0,), (last, 0, 5), (5, 2, 5, 0)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("key", list(CONFIGS))
def test_batched_frames_equal_the_eager_pictures_bitwise(torch_cuda, key, size):
    torch = torch_cuda
    from isaacgym_amd import render
    name, n = CONFIGS[key]
    task = make_plain(name, n, 4, episode_length=160)
    step = stepper(torch, task)
    w, h = size
    runs = []
    for sel in selections(n):
        for s in (1, 2, 4):
            r = render.Renderer(task, envs=sel, width=w, height=h, samples=s)
            cams = dict(side=render.Camera.side_view(r.scene), follow=render.Camera.follow_root(r.scene))
            runs.append(dict(r=r, cams=cams, traj=render.Trajectory(r, length=STEPS), eager={k: [] for k in cams}, posed=[], root=[]))
    for _ in range(STEPS):
        step()
        for run in runs:
            r = run["r"]
            for k, cam in run["cams"].items():
                r.set_camera(cam)
                run["eager"][k].append(r.render().clone())
            run["posed"].append(r.posed.clone())                                          # what pp_render_pose wrote for this step
            run["root"].append(r.scene.root[r.env_ids.long(), 0, :3].clone())
            run["traj"].capture()                                                         # under the follow-cam: its body is the anchor
    for run in runs:
        r, traj = run["r"], run["traj"]
        what = f"{key} {w}x{h} envs {r.envs} samples {r.samples}"
        posed, anchor, steps = traj.frames()
        assert steps == list(range(STEPS))
        assert torch.equal(posed, torch.stack(run["posed"]).view(torch.int32)), what
        assert torch.equal(anchor[..., :3], torch.stack(run["root"])) and not anchor[..., 3].any(), what
        for k, cam in run["cams"].items():
            want = torch.stack(run["eager"][k])
            r.set_camera(cam)
            assert torch.equal(traj.render(), want), f"{what} {k} (defaults)"
            r.set_camera(run["cams"]["side"])
            assert torch.equal(traj.render(camera=cam), want), f"{what} {k}"
        follow = torch.stack(run["eager"]["follow"])
        run["moving"] = not all(torch.equal(follow[0], f) for f in follow[1:])
    # a frozen anchor cannot pass: the anchors are compared with the root rows above, step by step, and the follow-cam pictures do change
    # (a 1 x 1 picture is one pixel, which five steps need not change: 0 to 3 of its 9 runs did when this was written)
    if w > 1:
        for run in runs:
            assert run["moving"], f"{key} {w}x{h} envs {run['r'].envs} samples {run['r'].samples}: the five follow-cam frames are all equal"
    if name == TA:                                                                        # the one floating base: its root, and so its anchor, moves
        assert all(not torch.equal(run["root"][0], run["root"][-1]) for run in runs), "no root moved: the anchor check shows nothing"


@pytest.mark.parametrize("s", [1, 2, 4])
def test_chunking_changes_nothing(torch_cuda, monkeypatch, s):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make_plain(TA, 64, 4, episode_length=160)
    step = stepper(torch, task)
    r = render.Renderer(task, envs=(63, 0, 5), width=33, height=17, samples=s, camera=None)
    r.set_camera(render.Camera.follow_root(r.scene))
    traj = render.Trajectory(r, length=STEPS)
    eager = []
    for _ in range(STEPS):
        step()
        eager.append(r.render().clone())
        traj.capture()
    one = traj.render()
    assert render.launch_frames(s, 3, 33, 17) >= STEPS and torch.equal(one, torch.stack(eager))
    rays = 3 * 33 * 17 * s * s
    for per_launch in (1, 2):
        monkeypatch.setattr(render, "MAX_LAUNCH_RAYS", per_launch * rays)
        assert render.launch_frames(s, 3, 33, 17) == per_launch
        assert torch.equal(traj.render(), one), f"{per_launch} frame(s) per launch"
    monkeypatch.setattr(render, "MAX_LAUNCH_RAYS", 1)                                     # below one frame: still one frame per launch
    assert render.launch_frames(s, 3, 33, 17) == 1 and torch.equal(traj.render(), one)


def test_an_env_id_out_of_range_records_an_empty_scene_and_a_zero_anchor(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import _lib, render
    task = make_plain(TT, 64, 4, episode_length=160)
    step = stepper(torch, task)
    for _ in range(3):
        step()
    r = render.Renderer(task, envs=(0, 1, 2), width=33, height=17, samples=2)
    r.set_camera(render.Camera.follow_root(r.scene))
    r.env_ids = torch.tensor([0, 64, -1], dtype=torch.int32, device=DEV)                 # the kernels' own guard, past the constructor's
    eager = r.render().clone()
    sc = r.scene
    posed = torch.full((1, 3, len(sc.prims), render.POSED_WORDS), 7, dtype=torch.int32, device=DEV)
    anchor = torch.full((1, 3, 4), 7.0, dtype=torch.float32, device=DEV)
    _lib.check(r.L.pp_render_pose_anchor(C.byref(sc.header), sc.prims_dev.data_ptr(), r.env_ids.data_ptr(), 3, render.SRC_ROOT, 0, posed.data_ptr(),
                                         anchor.data_ptr(), _lib.stream(DEV)), r.L)
    out = torch.zeros((1,) + tuple(eager.shape), dtype=torch.uint8, device=DEV)
    render.cast_frames(r.L, sc.header, r._cam, posed, anchor, 2, out)
    torch.cuda.synchronize()
    assert torch.equal(anchor[0, 0, :3], sc.root[0, 0, :3]) and not anchor[0, 1:].any() and float(anchor[0, 0, 3]) == 0.0
    assert torch.equal(posed[0], r.posed.view(torch.int32)) and bool((posed[0, 1:, :, 7] == -1).all())
    assert torch.equal(out[0], eager)
    assert torch.equal(eager[1], eager[2]) and not torch.equal(eager[0], eager[1])        # sky and ground alone


def test_ring_wrap_and_the_deferred_recorder(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make_plain(TA, 64, 4, episode_length=160)
    step = stepper(torch, task)
    r = render.Renderer(task, envs=(0, 5), width=33, height=17, samples=2)
    eager, deferred, traj = render.Recorder(r, 3, 2), render.Recorder(r, 3, 2, deferred=True), render.Trajectory(r, 3, 2)
    assert eager.trajectory is None and deferred.trajectory is not None
    for k in range(11):
        step()
        for rec in (eager, deferred, traj):
            rec.capture()
        if k == 6:                                                                        # a read in the middle draws what is there; the rest later
            assert torch.equal(deferred.frames(), eager.frames())
    rendered, kept = render.ring_schedule(11, 3, 2)
    assert kept == [6, 8, 10] and traj.frames()[2] == kept and deferred.trajectory.frames()[2] == kept
    assert (eager.captured, deferred.captured, traj.captured) == (rendered,) * 3 and deferred.calls == 11
    want = eager.frames()
    assert tuple(want.shape) == (3, 2, 17, 33, 4) and not torch.equal(want[0], want[-1])
    assert torch.equal(deferred.frames(), want) and torch.equal(traj.render(), want)
    assert torch.equal(deferred.frames(), want)                                           # again: nothing is pending


def test_re_rendering_is_rendering_also_from_a_file_without_the_task(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make_plain(TA, 64, 4, episode_length=160)
    step = stepper(torch, task)
    small = render.Renderer(task, envs=(63, 0, 5), width=32, height=24)
    big = render.Renderer(task, envs=(63, 0, 5), width=64, height=48, samples=2)
    follow = render.Camera.follow_root(big.scene)
    big.set_camera(follow)
    traj = render.Trajectory(small, length=STEPS)
    eager, first = [], []
    for _ in range(STEPS):
        step()
        first.append(small.render().clone())
        eager.append(big.render().clone())
        traj.capture()
    want, first = torch.stack(eager), torch.stack(first)
    assert torch.equal(traj.render(camera=follow, width=64, height=48, samples=2), want)
    path = traj.save(str(tmp_path / "rally.traj.npz"), fps=25)
    del traj, small, big, step, task
    gc.collect()
    rep = render.Replay.load(path, DEV)
    assert rep.meta["task"] == TA and rep.envs == [63, 0, 5] and rep.steps == list(range(STEPS)) and rep.fps == 25
    assert torch.equal(rep.render(camera=follow, width=64, height=48, samples=2), want)
    assert torch.equal(rep.render(camera=rep.camera("follow"), width=64, height=48, samples=2), want)
    assert torch.equal(rep.render(), first)                                               # the defaults: the recording's own camera, size, samples
    assert torch.equal(rep.render(camera=rep.camera("side")), first)                      # ... which was the side view
    files = rep.save(str(tmp_path / "again.npy"), width=16, height=16)
    assert np.load(files[0]).shape == (STEPS, 16, 3 * 16, 3)


def test_training_with_deferred_capture_is_the_same_run_and_writes_the_same_files(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd import render
    runs = {}
    for mode in ("off", "eager", "deferred"):
        tr = make_trainer(TA, 128)
        cap = None
        if mode != "off":
            r = render.Renderer(tr.task, envs=[0, 5], width=64, height=48, samples=2)
            kw = dict(deferred=True, trajectories=True) if mode == "deferred" else {}
            cap = render.TrainingCapture(r, str(tmp_path / mode), freq=16, length=8, ext=".npy", **kw)
            tr.set_capture(cap)
        for e in range(2):
            if e > 0:
                torch.cuda.set_sync_debug_mode("error")                                   # recordings open and end inside this epoch
            try:
                tr.train_epoch()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            if cap is not None:
                cap.poll()
        runs[mode] = (whole_state(torch, tr), cap.close() if cap is not None else [])
    assert runs["off"][0] == runs["eager"][0] == runs["deferred"][0]
    opened = (0, 16, 32, 48)
    assert [os.path.basename(p) for p in runs["eager"][1]] == [f"rl-video-step-{k}.npy" for k in opened]
    assert sorted(os.path.basename(p) for p in runs["deferred"][1]) == sorted([f"rl-video-step-{k}.npy" for k in opened] +
                                                                              [f"rl-video-step-{k}.traj.npz" for k in opened])
    for k in opened:
        want = np.load(tmp_path / "eager" / f"rl-video-step-{k}.npy")
        got = np.load(tmp_path / "deferred" / f"rl-video-step-{k}.npy")
        assert want.shape == (8, 48, 128, 3) and np.array_equal(got, want), f"recording {k}"
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 4                             # a picture, not a blank
        rep = render.Replay.load(str(tmp_path / "deferred" / f"rl-video-step-{k}.traj.npz"), DEV)
        assert rep.steps == list(range(k, k + 8)) and rep.envs == [0, 5]
        again = render.save_frames(rep.render().cpu().numpy(), str(tmp_path / f"replay-{k}.npy"))
        assert np.array_equal(np.load(again[0]), want), f"replay of recording {k}"


def test_player_with_a_deferred_recorder(torch_cuda, checkpoint):  # noqa: F811
    torch = torch_cuda
    from isaacgym_amd import render
    from isaacgym_amd.play import Player
    runs = []
    for deferred in (False, True):
        task = make_plain(TT, 8, 21)
        rec = render.Recorder(render.Renderer(task, envs=[0, 1], width=64, height=48), length=5, every=3, deferred=deferred)
        pl = Player(task, load_policy(checkpoint(TT)), games_num=4, poll_every=16, max_steps=2000, recorder=rec)
        runs.append((pl, pl.run(), rec))
    (pa, ra, reca), (pb, rb, recb) = runs
    strip = lambda res: {k: v for k, v in res.items() if k != "seconds"}      # noqa: E731
    assert strip(ra) == strip(rb) and ra["games"] >= 4 and ra["captured_frames"] == (ra["steps_played"] + 2) // 3
    assert pa.stats.state_bytes() == pb.stats.state_bytes()
    assert torch.equal(recb.frames(), reca.frames()) and tuple(reca.frames().shape) == (5, 2, 48, 64, 4)


def test_play_cli_deferred_with_a_trajectory_and_the_replay_cli(torch_cuda, checkpoint, tmp_path, capsys):  # noqa: F811
    from isaacgym_amd import play, render
    path, traj = str(tmp_path / "cli.gif"), str(tmp_path / "cli.traj.npz")
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "8", "--games", "4", "--poll-every", "16", "--seed", "3", "--capture", path,
                     "--capture-envs", "0,1", "--capture-len", "4", "--capture-every", "2", "--capture-size", "72x40", "--camera", "follow",
                     "--capture-deferred", "--capture-trajectory", traj])
    out = capsys.readouterr().out
    assert res["captured_frames"] == (res["steps_played"] + 1) // 2 and "captured" in out and "(trajectory)" in out
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(path)
    assert im.size == (144, 40) and 1 <= im.n_frames <= 4
    second = str(tmp_path / "replay.gif")
    files = render.main(["replay", traj, "--out", second, "--size", "48x32", "--samples", "2", "--camera", "side"])
    assert files == [second] and "replayed 4 frames" in capsys.readouterr().out
    im = Image.open(second)
    assert im.size == (96, 32) and 1 <= im.n_frames <= 4


@pytest.mark.parametrize("name,s", [(TT, 1), (TA, 4)], ids=["TT-s1", "TA-s4"])
def test_recording_and_casting_replay_in_a_captured_graph(torch_cuda, name, s):
    torch = torch_cuda
    from isaacgym_amd import _lib, render
    task = make_plain(name, 8, 4, episode_length=160)
    step = stepper(torch, task)
    for _ in range(3):
        step()
    r = render.Renderer(task, envs=[0, 6], width=72, height=40, samples=s)
    r.set_camera(render.Camera.follow_root(r.scene))
    sc = r.scene
    posed = torch.zeros((1, 2, len(sc.prims), render.POSED_WORDS), dtype=torch.int32, device=DEV)
    anchor = torch.zeros((1, 2, 4), dtype=torch.float32, device=DEV)
    out = torch.zeros((1, 2, 40, 72, 4), dtype=torch.uint8, device=DEV)

    def pair():
        sc.refresh()
        _lib.check(r.L.pp_render_pose_anchor(C.byref(sc.header), sc.prims_dev.data_ptr(), r.env_ids.data_ptr(), 2, render.SRC_ROOT, 0, posed.data_ptr(),
                                             anchor.data_ptr(), _lib.stream(DEV)), r.L)
        render.cast_frames(r.L, sc.header, r._cam, posed, anchor, s, out)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        pair()                                                                            # warm-up on the capture stream
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pair()
    before = out.clone()
    for _ in range(4):
        step()
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = r.render().clone()
    torch.cuda.synchronize()
    assert torch.equal(replayed[0], eager)
    assert not torch.equal(replayed, before)
