"""render.TrainingCapture without a GPU: its schedule (gym's RecordVideo rule: a step k with k % freq == 0 outside a recording opens one of
`length` steps, every `every`-th drawn) against a plain restatement written here, the files and their frames with a fake renderer on the
CPU, the writer's hand-over, and the refusals."""
import os
import types

import numpy as np
import pytest
import torch

from isaacgym_amd import render
from isaacgym_amd.collector import RolloutCollector
from isaacgym_amd.ppo import PPOTrainer


class FakeRenderer:
    """Renderer's surface for a TrainingCapture, on the CPU: a frame is filled with the number of the control step it is drawn after."""

    def __init__(self, shape=(2, 4, 6, 4), task=None):
        self.rgba, self.device, self.task = torch.zeros(shape, dtype=torch.uint8), torch.device("cpu"), task
        self.step, self.drawn = None, []

    def render(self, out=None):
        out.fill_(self.step % 251)
        self.drawn.append(self.step)
        return out


def rule(steps, freq, length, every, start=0):
    """{k of the opening step: [k of every drawn step]}, step by step as the rule is worded."""
    out, open_at = {}, None
    for k in range(start, start + steps):
        if open_at is None and k % freq == 0:
            open_at = k
            out[k] = []
        if open_at is not None:
            if (k - open_at) % every == 0:
                out[open_at].append(k)
            if k - open_at + 1 == length:
                open_at = None
    return out


def run(tmp_path, steps, start=0, poll_at=(), **kw):
    r = FakeRenderer()
    cap = render.TrainingCapture(r, str(tmp_path / "videos"), ext=".npy", start_step=start, **kw)
    polled = []
    for k in range(start, start + steps):
        r.step = k
        cap.on_step()
        if k in poll_at:
            polled.append((k, cap.poll()))
    return r, cap, polled


def check_files(cap, files, want):
    assert [os.path.basename(p) for p in files] == [f"rl-video-step-{k}.npy" for k in sorted(want)]
    for p, k in zip(files, sorted(want)):
        got = np.load(p)
        assert got.shape == (len(want[k]), 4, 2 * 6, 3)                                   # [T, H, E * W, 3]
        assert [int(f.flat[0]) for f in got] == [d % 251 for d in want[k]] and all((f == f.flat[0]).all() for f in got)


CASES = [dict(steps=96, freq=40, length=30, every=2),                                    # the GPU tests' schedule: 15, 15 and 8 frames
         dict(steps=100, freq=10, length=25, every=1),                                   # triggers at 10 and 20 fall inside the recording of 0
         dict(steps=70, freq=40, length=30, every=2, start=64),                          # a resumed run: the first recording is 80
         dict(steps=50, freq=16, length=16, every=3),                                    # back to back; 6 frames each; a short last one
         dict(steps=33, freq=1464, length=100, every=1),                                 # the reference's defaults, cut short
         dict(steps=45, freq=7, length=3, every=5, start=3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_schedule_against_the_rule_restated(tmp_path, case):
    case = dict(case)
    steps, start = case.pop("steps"), case.pop("start", 0)
    want = rule(steps, start=start, **case)
    r, cap, _ = run(tmp_path, steps, start=start, **case)
    assert r.drawn == [k for key in sorted(want) for k in want[key]]
    files = cap.close()
    check_files(cap, files, want)
    assert cap.close() == files and not cap.recording


def test_the_issue_s_numbers():
    want = rule(96, 40, 30, 2)
    assert {k: len(v) for k, v in want.items()} == {0: 15, 40: 15, 80: 8}
    assert list(rule(70, 40, 30, 2, start=64)) == [80, 120]
    assert list(rule(100, 10, 25, 1)) == [0, 30, 60, 90] and len(rule(100, 10, 25, 1)[90]) == 10


def test_poll_returns_what_is_finished_and_close_the_rest(tmp_path):
    r, cap, polled = run(tmp_path, 96, poll_at=(10, 29), freq=40, length=30, every=2)
    assert polled[0] == (10, [])                                                          # recording 0 is still open
    assert cap.recording                                                                  # ... and 80 is now
    files = cap.close()
    assert [os.path.basename(p) for p in files] == ["rl-video-step-0.npy", "rl-video-step-40.npy", "rl-video-step-80.npy"]
    assert all(os.path.exists(p) for p in files) and cap.poll() == files
    assert polled[1][1] in ([], files[:1])                                                # handed to the writer at step 29; it may not be done
    assert len(cap._free) <= 3 and all(b.shape == cap.recorder.ring.shape for b in cap._free)


def test_a_recording_that_ends_while_the_writer_holds_the_buffer_gets_another(tmp_path, monkeypatch):
    """Two recordings end without a poll() between them: the first one's frames must not be overwritten in host memory."""
    want = rule(40, 10, 8, 1)
    r, cap, _ = run(tmp_path, 40, freq=10, length=8, every=1)
    assert len(cap._in_flight) == 4 and len({id(j[2]) for j in cap._in_flight}) == 4
    check_files(cap, cap.close(), want)


def test_a_writer_error_is_raised_on_the_main_thread(tmp_path, monkeypatch):
    r, cap, _ = run(tmp_path, 10, freq=10, length=4, every=1)

    def boom(*a, **k):
        raise OSError("disk full")
    monkeypatch.setattr(render, "save_frames", boom)
    with pytest.raises(OSError, match="disk full"):
        cap.close()


def test_start_step_cannot_move_inside_a_recording(tmp_path):
    r, cap, _ = run(tmp_path, 3, freq=10, length=8)
    assert cap.recording and cap.start_step == 3
    with pytest.raises(RuntimeError, match="open"):
        cap.start_step = 64
    cap.close()
    cap.start_step = 64
    assert cap.start_step == 64


@pytest.mark.parametrize("kw", [dict(freq=0), dict(length=0), dict(every=0), dict(freq=2.5), dict(start_step=-1), dict(ext=".mp4")])
def test_bad_arguments(tmp_path, kw):
    with pytest.raises(ValueError):
        render.TrainingCapture(FakeRenderer(), str(tmp_path), **{"ext": ".npy", **kw})


def _trainer_stub(task, epoch=2, rank=0):
    return types.SimpleNamespace(task=task, rank=rank, epoch=epoch, cfg=types.SimpleNamespace(horizon_length=32), col=types.SimpleNamespace(on_step=None))


def test_set_capture_refuses_a_renderer_of_another_task_and_continues_the_numbering(tmp_path):
    mine, other = object(), object()
    tr = _trainer_stub(mine)
    with pytest.raises(ValueError, match="^the recorder renders another task$"):
        PPOTrainer.set_capture(tr, render.TrainingCapture(FakeRenderer(task=other), str(tmp_path), ext=".npy"))
    assert tr.col.on_step is None
    cap = render.TrainingCapture(FakeRenderer(task=mine), str(tmp_path), ext=".npy")
    PPOTrainer.set_capture(tr, cap)
    assert tr.col.on_step == cap.on_step and cap.start_step == 64
    PPOTrainer.set_capture(tr, None)
    assert tr.col.on_step is None
    rank1 = _trainer_stub(mine, rank=1)
    PPOTrainer.set_capture(rank1, cap)                                                    # rank 0 alone captures
    assert rank1.col.on_step is None


def test_the_collector_calls_on_step_after_every_env_step():
    """collect() with stand-ins for the env and the network (no kernel runs before the bootstrap forward raises the sentinel)."""
    calls = []

    class Stop(Exception):
        pass

    class Net:
        num_actions = 3

        def forward(self, obs, head_out=None, sample=None):
            if sample is None:
                raise Stop
            calls.append("forward")

    class Env:
        num_envs, num_rows, device, obs_buf = 2, 2, torch.device("cpu"), torch.zeros(2, 5)

        def step(self, actions, obs=None, rew=None, reset=None):
            calls.append("step")

    col = RolloutCollector(Env(), Net(), horizon=3)
    assert col.on_step is None
    with pytest.raises(Stop):
        col.collect()
    assert calls == ["forward", "step"] * 3
    calls.clear()
    col.on_step = lambda: calls.append("hook")
    with pytest.raises(Stop):
        col.collect()
    assert calls == ["forward", "step", "hook"] * 3
