"""Training with privileged critic inputs on the MI355X (PPOTrainer(critic_inputs=); RolloutCollector(critic_input=);
include/ppenv_critic_input.h): the collector's privileged rows are a torch gather of the env's tables, the delay lines' delays and the
undelayed observation as they stood after the step before; the run is finite, resumes bitwise, and its checkpoint plays; without the
argument the trainer is bitwise the trainer from before; two gloo ranks stay identical.  64 envs, horizon 4, minibatches of 64 rows, two
mini-epochs, 5-step games (every env resets inside a horizon or two).  Need a real MI355X."""
import os
import subprocess
import sys

import pytest

import dr_shim_binding as drb
from test_play_gpu import make_plain, torch_cuda        # noqa: F401  (a helper, a fixture)
from test_ppo_latency_gpu import learned_state, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TT, T4, TA = "HumanoidPingpongTiltG1", "Humanoid12PingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1"
H, SEED = 4, 21
DIMS = {"link_mass_scale": dict(start=(0.9, 1.1), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(1.0, 1.0), limit=(0.4, 1.6), step=0.1),
        "dof_damping_scale": dict(start=(0.8, 1.2), limit=(0.5, 2.0), step=0.1)}
ADR = dict(dims=DIMS, boundary_frac=0.5, min_games=1000, t_low=0.0, t_high=1e9)            # nothing is judged: fixed ranges, boundary workers
FULL = dict(action_delay=(0, 2), obs_delay=1, critic_inputs=("tables", "latency", "raw_obs"))


def trainer(name, num_envs=64, seed=SEED, **kw):
    """init_scale: the loss gradient per row is scale / minibatch_size times O(z / sigma) ~ 7 |advantage| |z| at sigma = exp(-2); at the
    yaml's 65536 / 8192 = 8 per row that is far inside fp16, at 65536 / 64 = 1024 per row it is at fp16's 65504 and the scaler spends the
    first steps backing off (a skipped step reports a non-finite grad_norm, with or without this feature).  The tests keep the yaml's
    scale PER ROW: 8 x 64 = 512."""
    from isaacgym_amd import ppo
    cfg = ppo.PPOConfig(horizon_length=H, minibatch_size=64, mini_epochs=2, init_scale=512.0)
    return ppo.PPOTrainer(make_plain(name, num_envs, seed, 5), cfg, seed=seed, **kw)


def expected_priv(torch, tr):
    """The privileged rows as a torch gather of what the env and the collector hold NOW."""
    col, env, A = tr.col, tr.env, tr.env.num_agents
    parts = []
    for name in tr.critic_inputs()["names"]:
        if name == "tables":
            parts += [t.reshape(-1, env.num_envs).t().repeat_interleave(A, 0) for t in env.dr_tables if t is not None]
        elif name == "latency":
            parts += [line.delays.float()[:, None] for line in (col.act_line, col.obs_line) if line is not None]
        else:
            parts.append(col.raw_obs)
    return torch.cat(parts, 1)


def watch(torch, tr):
    """on_step: after step t — the gather of row t + 1 has run — row t + 1 must be the torch gather of the sources as they stand."""
    seen = []

    def on_step():
        t = len(seen) % H
        want, got = expected_priv(torch, tr), tr.col.priv[t + 1]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), len(seen)
        seen.append(got.clone())
    tr.col.on_step = on_step
    return seen


def epochs(torch, tr, n):
    stats = [tr.train_epoch() for _ in range(n)]
    vals = torch.stack([v.detach().double() for s in stats for v in s.values() if v.dim() == 0])
    assert bool(torch.isfinite(vals).all())
    return vals


# ------------------------------------------------------------------------------------------------------ 5. end to end
def test_end_to_end_with_every_source_resumes_bitwise_and_plays(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd.policy import RLGamesPolicy
    a = trainer(TT, randomization=drb.mixed_plan(frequency=1), **FULL)
    rec = a.critic_inputs()
    assert rec == dict(names=["tables", "latency", "raw_obs"], columns=[23, 2, a.num_obs], P=25 + a.num_obs)
    P, col = rec["P"], a.col
    assert col.priv.shape == (H + 1, a.rows, P) and a.learner.num_priv == P and a.learner.net.w[0].shape[-1] == (a.num_obs + P + 63) // 64 * 64
    assert torch.equal(col.priv[0], expected_priv(torch, a))                                    # row 0: gathered at construction
    seen = watch(torch, a)
    epochs(torch, a, 1)
    assert torch.equal(col.priv[0], seen[H - 1])                                                # next_horizon carried row H to row 0
    epochs(torch, a, 1)
    assert len(seen) == 2 * H
    rows = torch.stack(seen)
    assert not torch.equal(rows[0, :, :23], rows[-1, :, :23]) and len(set(rows[:, :, 23].flatten().tolist())) == 3      # tables redrawn; delays 0, 1, 2
    assert float(a.learner.priv_rms.count) > 1 and bool((a.learner.w32[0][0][:, a.num_obs:] == 0).all())
    path = str(tmp_path / "nn" / "run.pth")
    a.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["critic_inputs"] == rec and ck["model"]["critic_mean_std.running_mean"].shape == (P,)
    assert ck["model"]["a2c_network.actor_mlp.0.weight"].shape[1] == a.num_obs and ck["model"]["a2c_network.critic_mlp.0.weight"].shape[1] == a.num_obs + P
    # the checkpoint plays: the actor as it stands, the privileged columns held at zero
    pol = RLGamesPolicy.load(path, DEV)
    obs = a.env.obs_buf.clone()
    act, _ = pol.act(obs, deterministic=True)
    mu, _ = a.roll_net.forward(obs)
    assert pol.num_priv == P and torch.equal(act, mu.clamp(-1.0, 1.0))
    a.col.on_step = None
    epochs(torch, a, 1)                                                                          # the uninterrupted third epoch
    want = learned_state(a)
    # a trainer in the same env state (it played the same two epochs), everything load() restores spoiled, then load and one epoch
    b = trainer(TT, randomization=drb.mixed_plan(frequency=1), **FULL)
    epochs(torch, b, 2)
    with torch.no_grad():
        for p in b.learner.parameters():
            p.add_(0.5)
        for m in b.opt.exp_avg + b.opt.exp_avg_sq:
            m.zero_()
        b.learner.priv_rms.running_mean.add_(1.0)
        b.learner.priv_rms.inv_std.mul_(2.0)
        b.opt.state.zero_()
    b.load(path)
    assert b.epoch == 2
    epochs(torch, b, 1)
    assert same(torch, learned_state(b), want)
    for k in ("running_mean", "running_var", "count", "mean", "inv_std"):
        assert torch.equal(getattr(b.learner.priv_rms, k), getattr(a.learner.priv_rms, k)), k
    # other privileged columns are refused, by name, before anything is overwritten
    other = trainer(TT, randomization=drb.mixed_plan(frequency=1), action_delay=(0, 2), obs_delay=1, critic_inputs=("tables", "latency"))
    before = learned_state(other)
    with pytest.raises(ValueError, match=rf"trained with P = {P} privileged columns .* this trainer has P = 25"):
        other.load(path)
    assert same(torch, learned_state(other), before) and other.epoch == 0
    with pytest.raises(ValueError, match="this trainer has P = 0"):
        trainer(TT).load(path)


@pytest.mark.parametrize("name, kw, columns", [(TA, dict(adr=ADR, critic_inputs=("tables",)), [27 + 28 + 1]),
                                               (T4, dict(action_delay=(0, 2), obs_delay=1, critic_inputs="latency"), [2])], ids=["27dof-tables", "four-actor-latency"])
def test_other_tasks_run_two_epochs_with_their_sources(torch_cuda, name, kw, columns):
    torch = torch_cuda
    tr = trainer(name, **kw)
    assert tr.critic_inputs()["columns"] == columns and tr.col.priv.shape == (H + 1, tr.rows, sum(columns)) and tr.rows == 64 * tr.env.num_agents
    assert torch.equal(tr.col.priv[0], expected_priv(torch, tr))
    seen = watch(torch, tr)
    epochs(torch, tr, 2)
    assert len(seen) == 2 * H and not torch.equal(seen[0], seen[-1])
    if tr.env.num_agents == 2:                                                                  # both rows of an env see the env's delays
        assert torch.equal(seen[-1][0::2], seen[-1][1::2])
    assert bool((tr.learner.w32[0][0][:, tr.num_obs:] == 0).all()) and bool((tr.learner.net.w[0][0][:, tr.num_obs:] == 0).all())


def test_refusals_name_the_argument(torch_cuda):
    with pytest.raises(ValueError, match="critic_inputs: 'tables' needs a run with randomisation"):
        trainer(TT, critic_inputs=("tables",))
    with pytest.raises(ValueError, match="critic_inputs: 'latency' needs a delay line"):
        trainer(TT, critic_inputs=("latency",))
    with pytest.raises(ValueError, match="critic_inputs: 'raw_obs' needs an obs_delay line"):
        trainer(TT, action_delay=2, critic_inputs=("raw_obs",))
    with pytest.raises(ValueError, match="critic_inputs: 'states' is not one of"):
        trainer(TT, critic_inputs="states")


# ------------------------------------------------------------------------------------------------------ 6. off is off
def test_empty_critic_inputs_is_the_trainer_without_the_argument(torch_cuda):
    torch = torch_cuda
    kw = dict(randomization=drb.mixed_plan(frequency=1), action_delay=(0, 2), obs_delay=1)
    a, b = trainer(TT, **kw), trainer(TT, critic_inputs=(), **kw)
    va, vb = epochs(torch, a, 2), epochs(torch, b, 2)
    assert torch.equal(va, vb) and same(torch, learned_state(a), learned_state(b))

    def flat(sd, out, prefix=""):
        for k, v in sd.items():
            if isinstance(v, dict):
                flat(v, out, f"{prefix}{k}.")
            elif isinstance(v, (list, tuple)) and v and torch.is_tensor(v[0]):
                out.update({f"{prefix}{k}.{i}": t for i, t in enumerate(v)})
            else:
                out[prefix + k] = v
        return out
    sa, sb = flat(a.state_dict(), {}), flat(b.state_dict(), {})
    assert list(sa) == list(sb) and not any("critic_inputs" in k or "critic_mean_std" in k for k in sa)
    for k in sa:
        assert torch.equal(sa[k], sb[k]) if torch.is_tensor(sa[k]) else sa[k] == sb[k], k
    for t in (a, b):
        assert t.col.priv is None and t.col.critic_input is None and t.critic_inputs() is None and t.learner.num_priv == 0 and t.learner.priv_rms is None
        assert len(t.learner.parameters()) == 2 * len(t.cfg.units) + 4 and t.learner.net.w[0].shape[-1] == (t.num_obs + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------------ 7. data-parallel
def test_two_ranks_stay_identical_and_the_actors_privileged_columns_stay_zero(tmp_path):
    import torch
    worker = os.path.join(ROOT, "tests", "critic_input_dp_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc_per_node=2", worker, "--out", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    r0, r1 = (torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2))
    assert r0["world"] == r1["world"] == 2
    for key in ("params", "exp_avg", "exp_avg_sq", "start_stats"):
        assert len(r0[key]) == len(r1[key]) and all(torch.equal(x, y) for x, y in zip(r0[key], r1[key])), key
    assert torch.equal(r0["scaler"], r1["scaler"])
    for r in (r0, r1):
        assert r["actor_priv32"].shape == (2048, 9) and not r["actor_priv32"].any() and not r["actor_priv16"].any()
        assert r["params"][0].shape == (2048, 80) and r["params"][1].shape == (2048, 89)
    assert torch.equal(r0["critic_priv32"], r1["critic_priv32"]) and bool(r0["critic_priv32"].any())
    assert not torch.equal(r0["priv"], r1["priv"])                                              # each rank gathered its own shard's tables and delays
