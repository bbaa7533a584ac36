"""Training under reset-time domain randomisation or ADR on the MI355X (PPOTrainer(randomization=, adr=); RolloutCollector(randomizer=);
include/ppenv_dr.h, include/ppenv_dr_adr.h).

With neither argument the trainer is bitwise the trainer without them.  A fixed plan: the env's tables are the host build of the plan
(dr_shim_binding.HostDR) driven by the dones the collector recorded, and a column changes only in the steps where its env reset.  ADR: its
ranges, per-slot state and tables after three epochs are the numpy rule (adr_shim_binding.NumpyAdr) replayed on the rewards and dones
on_step saw, exactly; runs are reproducible per seed; the state survives save / load; two gloo ranks hold the same ranges, those of the
numpy update on the sum of their totals.  The tasks run with env.episodeLength 12.  Need a real MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adr_shim_binding as ab
import dr_shim_binding as drb
from isaacgym_amd import scene
from test_play_gpu import make_plain, make_randomized, torch_cuda        # noqa: F401  (helpers, a fixture)
from test_ppo_latency_gpu import learned_state, same
from test_serve_plan_gpu import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT, T4, TA = "HumanoidPingpongTiltG1", "Humanoid12PingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1"
H = 8
SEED = 21
TABLES_SEED = scene.stream_seed(SEED, scene.STREAM_TABLES)
DIMS = {"link_mass_scale": dict(start=(0.9, 1.1), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(1.0, 1.0), limit=(0.4, 1.6), step=0.1)}
# One threshold for both moves: every boundary that has gathered min_games games moves outward (mean >= T_MOVE) or back in (mean <= T_MOVE).
# T_MOVE lies between the boundary slots' mean returns of a dry run of test_adr_state_is_the_numpy_rule_on_the_record's trainer: the
# untrained policy's 12-step games on the 7-dof task all end at step 12 (uncredited, they began before the fill) and at step 24, where the
# four boundary slots scored 0.613, 0.689, 0.625 and 0.713 over 7 .. 10 games each.  The test checks under NumpyAdr that both moves occur.
T_MOVE = 0.65
ADR = dict(dims=DIMS, boundary_frac=0.5, min_games=2, t_low=T_MOVE, t_high=T_MOVE)


def trainer(name, num_envs, seed=SEED, episode_length=12, **kw):
    from isaacgym_amd import ppo
    return ppo.PPOTrainer(make_plain(name, num_envs, seed, episode_length), ppo.PPOConfig(horizon_length=H, minibatch_size=256), seed=seed, **kw)


def run_epochs(torch, epochs=2, **kw):
    tr = trainer(TT, 64, **kw)
    stats = [tr.train_epoch() for _ in range(epochs)]
    vals = torch.stack([v.detach().double() for s in stats for v in s.values() if v.dim() == 0])
    return tr, learned_state(tr), vals


def env_tables(tr):
    """{name: [rows, N] uint32 words} of the tables the env's step reads now."""
    return {name: bits(t.reshape(-1, tr.env.num_envs)) for name, t in zip(tr.env.DR_TABLE_ROWS, tr.env.dr_tables) if t is not None}


# ------------------------------------------------------------------------------------------------------ a. neither argument
def test_neither_argument_is_the_trainer_without_them(torch_cuda):
    torch = torch_cuda
    tr0, state0, vals0 = run_epochs(torch)
    tr, state, vals = run_epochs(torch, randomization=None, adr=None)
    assert same(torch, state, state0) and torch.equal(vals, vals0)
    for t in (tr, tr0):
        assert t.col.randomizer is None and t.adr is None and t.randomization is None and t.env.dr_tables is None
        sd = t.state_dict()
        assert "randomization" not in sd and "adr" not in sd
        assert not any(k.startswith("adr") for k in t.train_epoch())
        t.clear_randomization()


# ------------------------------------------------------------------------------------------------------ b. a fixed plan
@pytest.mark.parametrize("name, num_envs", [(TT, 64), (T4, 32)], ids=["tilt", "four-actor"])
def test_fixed_plan_in_training(torch_cuda, tmp_path, name, num_envs):
    torch = torch_cuda
    plan = drb.mixed_plan()
    tr = trainer(name, num_envs, randomization=plan)
    rr, col, A, n = tr.env.reset_randomization, tr.col, tr.env.num_agents, num_envs
    assert rr is col.randomizer and tr.randomization is plan and tr.adr is None
    host = drb.HostDR(plan, n, seed=TABLES_SEED, env_id_offset=0, reset_rows=A)
    host.apply(np.zeros(A * n, np.int64))                                                      # the trainer's first application: every env drawn
    same_tables = lambda: all(np.array_equal(w, host.tables[k].view(np.uint32)) for k, w in env_tables(tr).items())
    assert same_tables() and set(env_tables(tr)) == set(plan["tables"]) and int(rr.draws.sum()) == n
    seen = {"steps": 0, "dones": 0, "before": env_tables(tr)}

    def on_step():
        t = seen["steps"] % H
        done = col.dones[t].cpu().numpy()
        host.apply(done)
        now = env_tables(tr)
        assert same_tables(), seen["steps"]
        fired = done[::A] != 0
        seen["dones"] += int(fired.sum())
        for k in now:                                                                          # a column changes only in steps where its env reset
            assert np.array_equal(now[k][:, ~fired], seen["before"][k][:, ~fired]), (seen["steps"], k)
        seen["before"] = now
        seen["steps"] += 1
    col.on_step = on_step
    for _ in range(2):
        tr.train_epoch()
    assert seen["steps"] == 2 * H and seen["dones"] >= n                                       # 16 steps of 12-step episodes: every env restarted
    assert np.array_equal(rr.draws.cpu().numpy(), host.draws) and int(host.draws.max()) >= 2
    path = str(tmp_path / "dr.pth")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["randomization"]["frequency"] == 5 and ck["randomization"]["tables"]["friction_scale"]["range"] == [0.7, 1.3] and "adr" not in ck
    tr.clear_randomization()
    col.on_step = None
    assert col.randomizer is None and tr.randomization is None and tr.env.dr_tables is None and "randomization" not in tr.state_dict()
    draws = rr.draws.clone()
    tr.train_epoch()
    assert torch.equal(rr.draws, draws)


# ------------------------------------------------------------------------------------------------------ c. ADR
def dims_list(tr, dims):
    from isaacgym_amd import adr
    return [ab.dim(max(tr.env.DR_TABLE_ROWS[k], 1), v["start"], v["limit"], v["step"]) for k, v in adr.check_dims(dims).items()]


def record(tr):
    """on_step: the rewards and dones of every step and ADR's slots after it."""
    seen = []

    def on_step():
        t = len(seen) % H
        seen.append((tr.col.rewards[t].clone(), tr.col.dones[t].clone(), tr.adr.slot.clone()))
    tr.col.on_step = on_step
    return seen


def replay(tr, seen, args, seed=TABLES_SEED):
    """The numpy rule on the record, horizon by horizon."""
    a, A = tr.adr, tr.env.num_agents
    ref = ab.NumpyAdr(a.num_envs, dims_list(tr, args["dims"]), reset_rows=A, num_agents=A, seed=seed, env_id_offset=0,
                      **{k: args[k] for k in ("boundary_frac", "min_games", "t_low", "t_high")})
    n = a.num_envs
    fin_slot, fin_q = np.full((H, n), -1, np.int32), np.zeros((H, n), np.int64)
    for k, (rew, done, slot) in enumerate(seen):
        r = k % H
        ref.step(rew.cpu().numpy(), done.cpu().numpy(), fin_slot[r], fin_q[r])
        assert np.array_equal(ref.slot, slot.cpu().numpy()), k
        if r == H - 1:
            ref.update(ref.fold(fin_slot, fin_q))
    return ref


def assert_state_is(tr, ref):
    a = tr.adr
    for k in ab.STATE:
        t = getattr(a, k)
        assert np.array_equal(bits(t) if t.element_size() == 4 else t.cpu().numpy().view(np.uint64), ref.words()[k]), k
    got = env_tables(tr)
    assert list(got) == a.names
    for d, name in enumerate(a.names):
        assert np.array_equal(got[name], ref.tables[d].view(np.uint32)), name


def test_adr_state_is_the_numpy_rule_on_the_record(torch_cuda):
    torch = torch_cuda
    tr = trainer(TT, 64, adr=ADR)
    a = tr.adr
    assert a is tr.col.randomizer and a.D == 2 and a.slots == 5 and a.horizon == H and a.seed == TABLES_SEED and a.names == ["link_mass_scale", "friction_scale"]
    assert (a.slot == -1).all() and torch.equal(a.range, torch.tensor([[0.9, 1.1], [1.0, 1.0]], device=a.range.device))
    seen = record(tr)
    for _ in range(3):
        out = tr.train_epoch()
    assert out["adr_lo"].shape == out["adr_hi"].shape == (2,) and out["adr_games"].shape == out["adr_mean"].shape == (5,)
    assert torch.equal(out["adr_lo"], a.range[:, 0]) and torch.equal(out["adr_hi"], a.range[:, 1]) and torch.equal(out["adr_games"], a.games)
    ref = replay(tr, seen, ADR)
    assert len(seen) == 3 * H
    assert_state_is(tr, ref)
    print("adr slots: games", ref.games.tolist(), "mean", ref.mean.tolist(), "widened", ref.widened.tolist(), "narrowed", ref.narrowed.tolist(),
          "range", ref.range.tolist())
    assert int(ref.widened.sum()) >= 1 and int(ref.narrowed.sum()) >= 1 and int(ref.games.sum()) > 0     # under NumpyAdr: both moves occur
    tr.clear_randomization()
    tr.col.on_step = None
    assert tr.adr is None and tr.col.randomizer is None and tr.env.dr_tables is None
    assert not any(k.startswith("adr") for k in tr.train_epoch())


# ------------------------------------------------------------------------------------------------------ d. seeds
def test_adr_runs_are_reproducible_per_seed(torch_cuda):
    torch = torch_cuda
    tr_a, a, vals_a = run_epochs(torch, epochs=3, adr=ADR)
    tr_b, b, vals_b = run_epochs(torch, epochs=3, adr=ADR)
    assert same(torch, a, b) and torch.equal(vals_a, vals_b) and torch.isfinite(vals_a).all()
    for k in ab.STATE:
        assert torch.equal(getattr(tr_a.adr, k), getattr(tr_b.adr, k)), k
    for name in tr_a.adr.names:
        assert torch.equal(tr_a.adr.tables[name], tr_b.adr.tables[name]), name
    tr_c = trainer(TT, 64, seed=SEED + 1, adr=ADR)
    for _ in range(3):
        tr_c.train_epoch()
    assert not torch.equal(tr_c.adr.slot, tr_a.adr.slot) and not torch.equal(tr_c.adr.tables["link_mass_scale"], tr_a.adr.tables["link_mass_scale"])


# ------------------------------------------------------------------------------------------------------ e. checkpoints
def test_checkpoint_restores_ranges_and_accumulators_and_other_dims_raise(torch_cuda, tmp_path):
    torch = torch_cuda
    args = dict(ADR, min_games=1000)                                                           # nothing is judged: the accumulators hold the games
    tr = trainer(TT, 64, adr=args)
    for _ in range(3):                                                                         # the games that count end at step 24
        tr.train_epoch()
    tr.adr.range.copy_(torch.tensor([[0.85, 1.15], [0.9, 1.2]]))                               # ranges that have moved
    path = str(tmp_path / "adr.pth")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)["adr"]
    assert (ck["boundary_frac"], ck["min_games"], ck["t_low"], ck["t_high"]) == (0.5, 1000, T_MOVE, T_MOVE)
    assert ck["dims"]["friction_scale"] == {"start": [1.0, 1.0], "limit": [0.4, 1.6], "step": 0.1} and list(ck["dims"]) == ["link_mass_scale", "friction_scale"]
    assert int(ck["acc_n"].sum()) > 0
    fresh = trainer(TT, 64, adr=args)
    assert int(fresh.adr.games.sum()) == 0
    fresh.load(path)
    for k in ("range", "acc_n", "acc_q", "games", "dropped", "mean", "widened", "narrowed"):
        assert torch.equal(getattr(fresh.adr, k), getattr(tr.adr, k)), k
    assert fresh.epoch == 3 and (fresh.adr.slot == -1).all()                                    # the envs restart: per-env state is not checkpointed
    fresh.train_epoch()
    other = trainer(TT, 64, adr=dict(args, dims={"friction_scale": DIMS["friction_scale"]}))
    before = learned_state(other)
    with pytest.raises(ValueError, match="other dims"):
        other.load(path)
    assert same(torch, learned_state(other), before) and other.epoch == 0                       # refused before anything was overwritten
    plain = trainer(TT, 64)
    plain.load(path)                                                                           # a trainer without ADR reads the rest
    assert plain.epoch == 3


# ------------------------------------------------------------------------------------------------------ f. refusals
def test_both_arguments_and_a_randomize_true_task_raise(torch_cuda):
    from isaacgym_amd import ppo
    cfg = ppo.PPOConfig(horizon_length=H, minibatch_size=256)
    with pytest.raises(ValueError, match="randomization together with adr"):
        ppo.PPOTrainer(make_plain(TT, 64, SEED), cfg, seed=SEED, randomization=drb.mixed_plan(), adr=ADR)
    task = make_randomized(TT, 64, SEED)
    for kw in ({}, dict(adr=ADR), dict(randomization=drb.mixed_plan())):
        with pytest.raises(ValueError, match="task.randomize: True is not supported by PPOTrainer"):
            ppo.PPOTrainer(task, cfg, seed=SEED, **kw)
    with pytest.raises(ValueError, match="no table 'mass'"):
        ppo.PPOTrainer(make_plain(TT, 64, SEED), cfg, seed=SEED, adr=dict(ADR, dims={"mass": DIMS["friction_scale"]}))
    with pytest.raises(ValueError, match="name no actor parameter"):
        ppo.PPOTrainer(make_plain(TT, 64, SEED), cfg, seed=SEED, randomization=True)           # the default cfg carries no randomization_params
    from isaacgym_amd.adr import AutoRandomizer
    for kw in (dict(adr=ADR), dict(randomization=drb.mixed_plan())):                           # an env that already has tables or a plan
        tr = ppo.PPOTrainer(make_plain(TT, 64, SEED), cfg, seed=SEED, **kw)
        with pytest.raises(ValueError, match="already has randomisation tables or a reset-time plan"):
            AutoRandomizer(tr.env, DIMS)


# ------------------------------------------------------------------------------------------------------ g. the 27-dof and the 4-actor task
@pytest.mark.parametrize("name, num_envs", [(TA, 64), (T4, 32)], ids=["27dof", "four-actor"])
def test_other_tasks_run_an_epoch_under_adr(torch_cuda, name, num_envs):
    dims = dict(DIMS, dof_damping_scale=dict(start=(0.8, 1.2), limit=(0.5, 2.0), step=0.1))
    args = dict(ADR, dims=dims)
    tr = trainer(name, num_envs, episode_length=5, adr=args)                                  # 5-step games: every env resets inside the one horizon
    assert tr.adr.rows == ([27, 28, 1] if name == TA else [7, 7, 1]) and tr.adr.reset_rows == tr.env.num_agents
    seen = record(tr)
    tr.train_epoch()
    ref = replay(tr, seen, args)
    assert_state_is(tr, ref)
    assert len(seen) == H and int(ref.draws.sum()) >= 2 * num_envs and (ref.slot >= 0).all()


# ------------------------------------------------------------------------------------------------------ 5. data-parallel
def test_two_ranks_hold_the_ranges_of_the_summed_totals(tmp_path):
    import torch
    worker = os.path.join(ROOT, "tests", "adr_dp_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc_per_node=2", worker, "--out", str(tmp_path), "--t-move", str(T_MOVE)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    r0, r1 = (torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2))
    assert r0["world"] == r1["world"] == 2 and r0["offset"] == 0 and r1["offset"] == 64
    for k in ("range", "acc_n", "acc_q", "games", "dropped", "mean", "widened", "narrowed"):
        assert torch.equal(r0["state"][k], r1["state"][k]), k
    assert len(r0["own"]) == len(r1["own"]) == 2 and not torch.equal(r0["own"][1], r1["own"][1])   # each rank folded its own games
    assert int(r0["own"][1][0].sum()) == int(r1["own"][1][0].sum()) == 64                       # 16-step horizons: the 12-step games credited end at step 24
    ref = ab.NumpyAdr(1, [ab.dim(7, *(DIMS["link_mass_scale"][k] for k in ("start", "limit", "step"))), ab.dim(1, *(DIMS["friction_scale"][k] for k in ("start", "limit", "step")))],
                      boundary_frac=0.5, min_games=2, t_low=T_MOVE, t_high=T_MOVE)
    for a, b in zip(r0["own"], r1["own"]):
        ref.update((a + b).numpy())
    assert np.array_equal(r0["state"]["range"].numpy().view(np.uint32), ref.range.view(np.uint32))
    assert np.array_equal(r0["state"]["games"].numpy(), ref.games) and np.array_equal(r0["state"]["mean"].numpy().view(np.uint32), ref.mean.view(np.uint32))
    assert int(ref.games.sum()) == 128 and int(ref.widened.sum() + ref.narrowed.sum()) >= 1     # one threshold: every judged boundary moves one way
    assert np.array_equal(r0["state"]["widened"].numpy(), ref.widened) and np.array_equal(r0["state"]["narrowed"].numpy(), ref.narrowed)
