"""Videos recorded inside the training rollout on the MI355X (render.TrainingCapture under PPOTrainer.set_capture / fit / the CLI): a run
with capture is bitwise the run without, an epoch with a recording open still reads nothing on the host, the files hold the frames a
separate Renderer draws at the same steps of an identical run, a resumed run continues the numbering.  3 epochs of horizon 32 with
64 x 48 pictures, a recording of 30 steps every 40, every 2nd step drawn: files 0, 40 (across the epoch boundary at 64) and 80 (short).
Need a real MI355X."""
import os

import numpy as np
import pytest

from test_play_gpu import DEV, T4, TT, make_plain
from test_train_capture_host import rule

pytestmark = pytest.mark.gpu

TA = "HumanoidPingpongTiltNESSparse27DOFG1"
CONFIGS = [(TT, 64), (TA, 64), (T4, 32)]
EPOCHS, HORIZON, FREQ, LENGTH, EVERY = 3, 32, 40, 30, 2
SEL = [0, 5]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def make_trainer(name, num_envs, seed=3):
    from isaacgym_amd import ppo
    return ppo.PPOTrainer(make_plain(name, num_envs, seed), ppo.PPOConfig(minibatch_size=1024, save_best_after=1, games_to_track=10), seed=seed)


def make_capture(tr, out_dir, samples=2, **kw):
    from isaacgym_amd import render
    r = render.Renderer(tr.task, envs=SEL, width=64, height=48, samples=samples)
    return render.TrainingCapture(r, str(out_dir), freq=FREQ, length=LENGTH, every=EVERY, ext=".npy", **kw)


def tensors(x, out):
    import torch
    if torch.is_tensor(x):
        out.append(x.detach().cpu().numpy().tobytes())
    elif isinstance(x, dict):
        for k in sorted(x):
            tensors(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            tensors(v, out)
    else:
        out.append(repr(x).encode())
    return out


def whole_state(torch, tr):
    """Everything a checkpoint holds (parameters, Adam moments, scaler, lr, input and value statistics, meter, epoch, frame) plus the
    rollout's last observation and the running episodes, as bytes."""
    torch.cuda.synchronize()
    return tensors([tr.state_dict(), tr.col.obs[0], tr.ep_ret, tr.ep_len, tr.col.sigma, list(tr.meter.state_bytes())], [])


def epochs(torch, tr, k, after=None):
    out = []
    for e in range(k):
        if e > 0:
            torch.cuda.set_sync_debug_mode("error")                                    # epochs 1 and 2: a recording is open in both
            try:
                res = tr.train_epoch()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            res = tr.train_epoch()
        out.append(tensors(res, []))
        if after is not None:
            after()
    return out


@pytest.mark.parametrize("name,num_envs", CONFIGS, ids=["TT", "TA", "T4"])
def test_a_run_with_capture_is_the_same_run_and_its_files_hold_the_frames(torch_cuda, tmp_path, name, num_envs):
    torch = torch_cuda
    from isaacgym_amd import render
    want = rule(EPOCHS * HORIZON, FREQ, LENGTH, EVERY)
    assert {k: len(v) for k, v in want.items()} == {0: 15, 40: 15, 80: 8}
    a = make_trainer(name, num_envs)
    cap = make_capture(a, tmp_path / "videos")
    a.set_capture(cap)
    open_in = []
    stats_a = epochs(torch, a, EPOCHS, after=lambda: (open_in.append(cap.recording), cap.poll()))
    assert open_in == [False, True, True]                                              # 40 is open when epoch 1 ends, 80 when epoch 2 ends
    files = cap.close()
    b = make_trainer(name, num_envs)
    stats_b = epochs(torch, b, EPOCHS)
    assert stats_a == stats_b and len(stats_a[0]) >= 10
    assert whole_state(torch, a) == whole_state(torch, b)
    # the frames: an identical run whose own hook draws the scheduled steps with a Renderer of its own
    c = make_trainer(name, num_envs)
    r = render.Renderer(c.task, envs=SEL, width=64, height=48, samples=2)
    drawn, when, k = {}, {d: o for o, ds in want.items() for d in ds}, [0]

    def hook():
        if k[0] in when:
            drawn.setdefault(when[k[0]], []).append(r.render().clone())
        k[0] += 1
    c.col.on_step = hook
    epochs(torch, c, EPOCHS)
    assert k[0] == EPOCHS * HORIZON
    assert [os.path.basename(p) for p in files] == [f"rl-video-step-{o}.npy" for o in (0, 40, 80)]
    for p, o in zip(files, (0, 40, 80)):
        got = np.load(p)
        ref = render.save_frames(torch.stack(drawn[o]).cpu().numpy(), str(tmp_path / f"ref-{o}.npy"))
        assert got.shape == (len(want[o]), 48, 2 * 64, 3) and np.array_equal(got, np.load(ref[0])), f"recording {o}"
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 4                          # a picture, not a blank
    assert whole_state(torch, c) == whole_state(torch, b)


def test_a_resumed_run_continues_the_numbering_and_fit_returns_the_videos(torch_cuda, tmp_path):
    from isaacgym_amd import ppo
    a = make_trainer(TT, 64)
    first = ppo.fit(a, str(tmp_path), "run", print_every=0, max_epochs=2)
    assert "videos" not in first and first["epoch"] == 2
    b = make_trainer(TT, 64)
    b.load(first["paths"]["latest"])
    cap = make_capture(b, tmp_path / "videos")
    res = ppo.fit(b, str(tmp_path), "run", print_every=0, max_epochs=3, capture=cap)
    assert cap.start_step == 3 * HORIZON and b.col.on_step is None
    assert res["videos"] == [str(tmp_path / "videos" / "rl-video-step-80.npy")] and res["epoch"] == 3
    assert {k: v for k, v in res.items() if k != "videos"}.keys() == first.keys()
    assert np.load(res["videos"][0]).shape == (8, 48, 128, 3)
    with pytest.raises(ValueError, match="^the recorder renders another task$"):
        a.set_capture(cap)


def test_cli_writes_gifs_under_videos(torch_cuda, tmp_path, capsys):
    from isaacgym_amd import ppo
    res = ppo.main(["--task", TT, "--num-envs", "64", "--minibatch-size", "1024", "--max-epochs", "2", "--print-every", "0", "--out", str(tmp_path),
                    "--capture-video", "--capture-video-freq", "40", "--capture-video-len", "10", "--capture-size", "64x48", "--capture-envs", "0,1",
                    "--camera", "follow"])
    out = capsys.readouterr().out
    videos = tmp_path / "videos"
    assert res["videos"] == [str(videos / "rl-video-step-0.gif"), str(videos / "rl-video-step-40.gif")]
    assert sorted(os.listdir(videos)) == ["rl-video-step-0.gif", "rl-video-step-40.gif"] and out.count("(video)") == 2
    Image = pytest.importorskip("PIL.Image")
    for p in res["videos"]:
        im = Image.open(p)
        assert im.size == (128, 48) and 1 <= im.n_frames <= 10                        # PIL merges consecutive frames that are equal
    plain = ppo.main(["--task", TT, "--num-envs", "64", "--minibatch-size", "1024", "--max-epochs", "1", "--print-every", "0", "--out", str(tmp_path / "plain")])
    assert "videos" not in plain and not (tmp_path / "plain" / "videos").exists()
