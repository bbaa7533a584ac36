"""Training on a serve plan or an adaptive serve curriculum on the MI355X (PPOTrainer(serve_plan=, curriculum=); RolloutCollector(serve=);
include/ppenv_serve.h, include/ppenv_serve_curric.h).

With neither argument the trainer is bitwise the trainer without them.  A fixed plan: the serves consumed are the dones seen, the buffer
holds the host build's serve(e, count[e]), a reset consumes exactly the buffer's row, the checkpoint carries the cells.  A curriculum: its
table after three epochs is the numpy rule (serve_curric_shim_binding.NumpyCurric) replayed on the rewards and dones on_step saw, exactly;
runs are reproducible per seed; the table survives save / load.  The tasks run with env.episodeLength 12.  Need a real MI355X."""
import numpy as np
import pytest

import serve_curric_shim_binding as scb
import serve_shim_binding as ssb
from isaacgym_amd import _lib, scene, serve
from test_play_gpu import make_plain, torch_cuda        # noqa: F401  (a helper, a fixture)
from test_ppo_latency_gpu import learned_state, same
from test_serve_plan_gpu import ball_rows, bits

pytestmark = pytest.mark.gpu

TT, T4, TA = "HumanoidPingpongTiltG1", "Humanoid12PingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1"
FORM = {TT: scene.VARIANT_TT, T4: scene.VARIANT_T4, TA: scene.VARIANT_TN}
H = 8
SEED = 21
CELLS = [{"serve_speed": (6.0, 6.5), "serve_tilt": -3.0, "serve_tilt_z": (2.0, 9.0)}, {"serve_speed": (9.0, 9.5), "serve_tilt": (-5.0, 4.0), "serve_tilt_z": 6.0}]
GRID = {"serve_speed": (6.0, 9.0, 3), "serve_tilt": (-5.0, 5.0, 2)}


def trainer(name, num_envs, seed=SEED, **kw):
    from isaacgym_amd import ppo
    return ppo.PPOTrainer(make_plain(name, num_envs, seed), ppo.PPOConfig(horizon_length=H, minibatch_size=256), seed=seed, **kw)


def curriculum_args(**kw):
    from isaacgym_amd import curriculum
    return dict(dict(bins=curriculum.grid(GRID), power=2, mix=0.2, alpha=0.3), **kw)


def run_epochs(torch, epochs=2, **kw):
    tr = trainer(TT, 64, **kw)
    stats = [tr.train_epoch() for _ in range(epochs)]
    vals = torch.stack([v.detach().double() for s in stats for v in s.values() if v.dim() == 0])
    return tr, learned_state(tr), vals


# ------------------------------------------------------------------------------------------------------ 1. neither argument
def test_neither_argument_is_the_trainer_without_them(torch_cuda):
    torch = torch_cuda
    tr0, state0, vals0 = run_epochs(torch)
    tr, state, vals = run_epochs(torch, serve_plan=None, serve_paired=False, curriculum=None)
    assert same(torch, state, state0) and torch.equal(vals, vals0)
    for t in (tr, tr0):
        assert t.col.serve is None and t.curriculum is None and t.env.serve_plan is None and t.env.serve_curriculum is None and t.task._serve_plan is None
        sd = t.state_dict()
        assert "serve" not in sd and "curriculum" not in sd and t.serve() is None
        assert not any(k.startswith("curriculum") for k in t.train_epoch())


# ------------------------------------------------------------------------------------------------------ 2. a fixed plan
@pytest.mark.parametrize("name, num_envs", [(TT, 64), (T4, 32)], ids=["tilt", "four-actor"])
def test_fixed_plan_in_training(torch_cuda, tmp_path, name, num_envs):
    torch = torch_cuda
    tr = trainer(name, num_envs, serve_plan=CELLS)
    plan, col, A, n = tr.task._serve_plan, tr.col, tr.env.num_agents, num_envs
    assert plan is tr.env.serve_plan is col.serve
    assert int(plan.count.sum()) == 0 and tr.serve() == dict(cells=[{k: [float(v[0]), float(v[1])] for k, v in c.items()} for c in plan.cells], paired=False)
    seen = {"dones": 0, "resets": torch.zeros(n, dtype=torch.int64, device=tr.device), "before": plan.out.clone(), "steps": 0}

    def on_step():
        t = seen["steps"] % H
        fired = col.dones[t][::A] != 0
        seen["dones"] += int(fired.sum())
        seen["resets"] += fired
        if bool(fired.any()):                                                    # the row the buffer held BEFORE the step is the ball the reset served
            rows = ball_rows(tr.task, name)[fired]
            assert np.array_equal(bits(rows[:, 2:5]), bits(seen["before"][:, fired].T.contiguous())), seen["steps"]
        keep = ~fired
        assert np.array_equal(bits(plan.out[:, keep]), bits(seen["before"][:, keep])), seen["steps"]
        seen["before"] = plan.out.clone()
        seen["steps"] += 1
    col.on_step = on_step
    for _ in range(3):
        tr.train_epoch()
    assert seen["steps"] == 3 * H and int(plan.count.sum()) == seen["dones"] >= n                # 24 steps of 12-step episodes: every env restarted
    assert torch.equal(plan.count.to(torch.int64), seen["resets"])
    host = ssb.HostServe(n, CELLS, FORM[name], _lib.SERVE_LAYOUT_SOA3, reset_rows=A, seed=scene.stream_seed(SEED, scene.STREAM_SERVES), env_id_offset=0)
    host.count[:] = plan.count.cpu().numpy().view(np.uint32)
    host.fill()
    assert np.array_equal(bits(plan.out), host.out.view(np.uint32))                              # serve(e, count[e]) of the host build, bit for bit
    path = str(tmp_path / "serve.pth")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["serve"] == tr.serve() and ck["serve"]["cells"][0]["serve_tilt"] == [-3.0, -3.0] and "curriculum" not in ck
    tr.clear_serve()
    assert col.serve is None and tr.env.serve_plan is None and tr.task._serve_plan is None and "serve" not in tr.state_dict()
    count = plan.count.clone()
    col.on_step = None
    tr.train_epoch()                                                                           # the built-in serves: nothing advances the plan any more
    assert torch.equal(plan.count, count)


def test_a_task_that_arrives_with_a_plan_is_still_refused(torch_cuda):
    from isaacgym_amd import ppo
    task = make_plain(TT, 64, SEED)
    task.set_serve_plan(CELLS, paired=True)
    for kw in ({}, dict(serve_plan=CELLS), dict(curriculum=curriculum_args())):
        with pytest.raises(ValueError, match="clear_serve_plan"):
            ppo.PPOTrainer(task, ppo.PPOConfig(horizon_length=H, minibatch_size=256), seed=SEED, **kw)
    task.clear_serve_plan()
    tr = ppo.PPOTrainer(task, ppo.PPOConfig(horizon_length=H, minibatch_size=256), seed=SEED, serve_plan=CELLS, serve_paired=True)
    assert tr.col.serve is task._serve_plan and tr.serve()["paired"] is True
    for _ in range(2):                                                                         # 16 steps of 12-step episodes
        tr.train_epoch()
    assert int(task._serve_plan.count.sum()) >= 64


# ------------------------------------------------------------------------------------------------------ 3. the curriculum
def record(tr):
    """on_step: the rewards and dones of every step and the curriculum's cur_bin after it."""
    seen = []

    def on_step():
        t = len(seen) % H
        seen.append((tr.col.rewards[t].clone(), tr.col.dones[t].clone(), tr.curriculum.cur_bin.clone()))
    tr.col.on_step = on_step
    return seen


def replay(tr, name, seen, args):
    """The numpy rule on the record, horizon by horizon."""
    cur, A = tr.curriculum, tr.env.num_agents
    ref = scb.NumpyCurric(cur.num_envs, args["bins"], FORM[name], cur.layout, reset_rows=A, num_agents=A, seed=scene.stream_seed(SEED, scene.STREAM_SERVES),
                          env_id_offset=0, power=args["power"], mix=args["mix"], alpha=args["alpha"], defaults=tr.env.serve_defaults(),
                          axes=serve.AXES_27DOF if name == TA else serve.AXES_7DOF)
    n = cur.num_envs
    fin_bin, fin_q = np.full((H, n), -1, np.int32), np.zeros((H, n), np.int64)
    dones = uncounted = 0
    first = np.ones(n, bool)
    for k, (rew, done, cur_bin) in enumerate(seen):
        r = k % H
        d = done.cpu().numpy()
        ref.step(rew.cpu().numpy(), d, fin_bin[r], fin_q[r])
        assert np.array_equal(ref.cur_bin, cur_bin.cpu().numpy()), k
        fired = d[::A] != 0
        dones += int(fired.sum())
        uncounted += int((fired & first).sum())
        first &= ~fired
        if r == H - 1:
            ref.update(ref.fold(fin_bin, fin_q))
    return ref, dones, uncounted


@pytest.mark.parametrize("name, num_envs", [(TT, 64), (T4, 32)], ids=["tilt", "four-actor"])
def test_curriculum_table_is_the_numpy_rule_on_the_record(torch_cuda, name, num_envs):
    torch = torch_cuda
    args = curriculum_args()
    tr = trainer(name, num_envs, curriculum=args)
    cur = tr.curriculum
    assert cur is tr.env.serve_curriculum is tr.col.serve and cur.bins == 6 and cur.horizon == H and cur.seed == scene.stream_seed(SEED, scene.STREAM_SERVES)
    assert (cur.cur_bin == -1).all()
    seen = record(tr)
    for _ in range(3):
        out = tr.train_epoch()
    for k in ("curriculum_games", "curriculum_mean", "curriculum_prob"):
        assert out[k].shape == (6,) and out[k].device == cur.games.device
    assert torch.equal(out["curriculum_games"], cur.games) and abs(float(out["curriculum_prob"].sum()) - 1.0) < 1e-12
    ref, dones, uncounted = replay(tr, name, seen, args)
    assert len(seen) == 3 * H and uncounted == num_envs                                        # every env restarted, its first game uncounted
    assert np.array_equal(cur.games.cpu().numpy(), ref.games) and np.array_equal(cur.dropped.cpu().numpy(), ref.dropped)
    assert np.array_equal(bits(cur.mean), ref.mean.view(np.uint32)) and np.array_equal(cur.cdf.cpu().numpy().view(np.uint32), ref.cdf)
    assert int(cur.games.sum() + cur.dropped.sum()) == dones - uncounted > 0
    assert np.array_equal(cur.count.cpu().numpy().view(np.uint32), ref.count) and np.array_equal(cur.next_bin.cpu().numpy(), ref.next_bin)
    assert np.array_equal(bits(cur.out), ref.out.view(np.uint32))                              # the buffer: every env's next serve, from its bin's cell
    assert int((cur.games > 0).sum()) >= 4 and len(set(cur.cdf.tolist())) > 1
    # the Python surface is closed while the curriculum is set
    with pytest.raises(RuntimeError, match="inside collector steps only"):
        tr.task.step(tr.task.zero_actions())
    with pytest.raises(RuntimeError, match="inside collector steps only"):
        tr.task.reset_idx()
    with pytest.raises(ValueError, match="a serve curriculum is set"):
        tr.env.set_serve_plan(CELLS)
    tr.clear_serve()
    tr.col.on_step = None
    assert tr.curriculum is None and tr.env.serve_curriculum is None and tr.col.serve is None
    assert not any(k.startswith("curriculum") for k in tr.train_epoch())
    tr.task.step(tr.task.zero_actions())


def test_curriculum_runs_are_reproducible_per_seed(torch_cuda):
    torch = torch_cuda
    tr_a, a, vals_a = run_epochs(torch, epochs=3, curriculum=curriculum_args())
    tr_b, b, vals_b = run_epochs(torch, epochs=3, curriculum=curriculum_args())
    assert same(torch, a, b) and torch.equal(vals_a, vals_b) and torch.isfinite(vals_a).all()
    for k in ("games", "mean", "dropped", "cdf", "count", "next_bin", "cur_bin", "out"):
        assert torch.equal(getattr(tr_a.curriculum, k), getattr(tr_b.curriculum, k)), k
    tr_c = trainer(TT, 64, seed=SEED + 1, curriculum=curriculum_args())
    for _ in range(3):
        tr_c.train_epoch()
    assert not torch.equal(tr_c.curriculum.out, tr_a.curriculum.out) and not torch.equal(tr_c.curriculum.mean, tr_a.curriculum.mean)


def test_checkpoint_restores_the_table_and_other_bins_raise(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd import curriculum
    args = curriculum_args()
    tr = trainer(TT, 64, curriculum=args)
    for _ in range(2):
        tr.train_epoch()
    path = str(tmp_path / "curric.pth")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)["curriculum"]
    assert (ck["power"], ck["mix"], ck["alpha"]) == (2, 0.2, 0.3) and len(ck["bins"]) == 6 and ck["bins"][0]["serve_speed"] == [6.0, 7.0]
    assert set(ck["bins"][0]) == set(serve.AXES_7DOF) and set(ck) == {"bins", "power", "mix", "alpha", "games", "mean", "dropped", "cdf"}
    fresh = trainer(TT, 64, curriculum=args)
    assert int(fresh.curriculum.games.sum()) == 0
    fresh.load(path)
    for k in ("games", "mean", "dropped", "cdf"):
        assert torch.equal(getattr(fresh.curriculum, k), getattr(tr.curriculum, k)), k
    assert fresh.epoch == 2 and (fresh.curriculum.cur_bin == -1).all()                          # the envs restart: per-env state is not checkpointed
    fresh.train_epoch()
    other = trainer(TT, 64, curriculum=curriculum_args(bins=curriculum.grid({"serve_speed": (6.0, 9.0, 6)})))
    before = learned_state(other)
    with pytest.raises(ValueError, match="other bins"):
        other.load(path)
    assert same(torch, learned_state(other), before) and other.epoch == 0                       # refused before anything was overwritten
    plain = trainer(TT, 64)
    plain.load(path)                                                                           # a trainer without a curriculum reads the rest
    assert plain.epoch == 2


# ------------------------------------------------------------------------------------------------------ 4. the 27-dof task: the [N,5] rows
def test_27dof_curriculum_serves_the_buffers_rows(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import curriculum
    args = dict(bins=curriculum.grid({"serve_speed": (4.0, 6.0, 2), "ball_y": (-0.4, 0.0, 2)}), power=1, mix=0.25, alpha=0.5)
    n = 64
    tr = trainer(TA, n, curriculum=args)
    cur, col = tr.curriculum, tr.col
    assert cur.layout == _lib.SERVE_LAYOUT_AOS5 and tuple(cur.out.shape) == (n, 5) and cur.bins == 4
    seen = record(tr)
    state = {"before": cur.out.clone(), "count": cur.count.clone(), "served": 0}
    rec = col.on_step

    def on_step():
        rec()
        fired = seen[-1][1] != 0
        rows = tr.env.root_states[:, 2][:, [1, 2, 7, 8, 9]]
        assert np.array_equal(bits(rows[fired]), bits(state["before"][fired])), len(seen)        # ball y, z and velocity: the buffer's row before the step
        assert np.array_equal(bits(cur.out[~fired]), bits(state["before"][~fired])), len(seen)
        assert torch.equal(cur.count, state["count"] + fired.to(torch.int32))
        state["before"], state["count"] = cur.out.clone(), cur.count.clone()
        state["served"] += int(fired.sum())
    col.on_step = on_step
    for _ in range(3):
        tr.train_epoch()
    ref, dones, uncounted = replay(tr, TA, seen, args)
    assert state["served"] == dones == int(cur.count.sum()) >= n
    assert np.array_equal(cur.games.cpu().numpy(), ref.games) and np.array_equal(bits(cur.mean), ref.mean.view(np.uint32))
    assert np.array_equal(cur.cdf.cpu().numpy().view(np.uint32), ref.cdf) and np.array_equal(bits(cur.out), ref.out.view(np.uint32))
    assert int(cur.games.sum() + cur.dropped.sum()) == dones - uncounted > 0
