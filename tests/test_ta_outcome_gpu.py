"""The 27-dof task's outcome counts (include/ppenv_ta_outcome.h) on the GPU: the stateless entry over the golden fixture, the three step
kernels at ragged sizes, a captured step, the setter's off switch, the Player's latch and the trainer's statistics.

Expected values never come from the code under test: the count bits do not depend on the reset decision and a reset clears only the sticky
bits, so the bits "right before the clear" are what the same step leaves when max_episode_length is raised so that nobody resets — taken
from the unmodified oracle (the golden fixture) or from a step with the struct detached (the kernels)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ta_outcome_shim_binding as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TA = "HumanoidPingpongTiltNESSparse27DOFG1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_EP = 20                                          # episodeLength of the kernel cases: an env resets when progress + 1 >= L_EP - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def words(t):
    """pp_ta_outcome (an int64 [16] device tensor) as uint64 words on the host."""
    return t.cpu().numpy().view(np.uint64).copy()


# --------------------------------------------------------------------------------------------------- 1. the stateless entry, golden steps
def test_stateless_entry_over_the_golden_steps(torch_cuda, oracle_lib):
    torch = torch_cuda
    from isaacgym_amd import tensor_api
    from test_ta_golden import load, params_for
    e = B.golden_expectation(oracle_lib)
    g = load()
    p = params_for(g)
    T, n = g["out_rew"].shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    irb = dev(np.broadcast_to(g["initial_bodies42"], (n, 42, 13)).astype(np.float32))
    st, plain = tensor_api.TAState(p, device=DEV), tensor_api.TAState(p, device=DEV)
    out = torch.zeros(tensor_api.OUTCOME_WORDS, dtype=torch.int64, device=DEV)
    seen, unchanged = [], 0
    for t in range(T):
        ins = lambda: (dev(g["in_bodies42"][t]), irb, dev(g["in_root"][t]), dev(g["in_dof"][t]), dev(g["in_dof_force"][t]), dev(g["in_pre_vx"][t]))
        a, b = ins(), ins()
        before = words(out)
        st.post_physics_step(*a, reset_override=dev(np.nan_to_num(g["reset_override"][t])), outcome=out)
        plain.post_physics_step(*b, reset_override=dev(np.nan_to_num(g["reset_override"][t])))
        got = words(out)
        np.testing.assert_array_equal(got, e["structs"][t], err_msg=f"struct after step {t}")
        if e["resets"][t] == 0:
            assert got.tobytes() == before.tobytes()
            unchanged += 1
        seen.append((int(got[0]), int(got[1])))
        for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "flags", "episode", "_any_reset"):
            assert torch.equal(getattr(st, name), getattr(plain, name)), f"{name}, step {t}"
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), f"root / dof after reset, step {t}"
        np.testing.assert_array_equal(st.flags.cpu().numpy().view(np.uint32), g["out_flags"][t])
    assert unchanged == 34
    assert seen[11] == (0, 0) and seen[12] == (1, 32) and seen[24] == (1, 32) and seen[25] == (2, 64) and seen[-1] == (2, 64)
    last = words(out)
    np.testing.assert_array_equal(last[8:13], e["preclear"][25])              # last[] overwritten by the second window
    assert not np.array_equal(e["preclear"][25], e["preclear"][12])


# ------------------------------------------------------------------------------------------------------------- 2. the three step kernels
FIELDS = ("root_states", "dof_states", "_rb_states", "dof_force_tensor", "pre_ball_vx")
STATE = ("flags", "episode", "progress_buf", "obs_buf", "rew_buf", "reset_buf", "_any_reset")


def snapshot(env):
    s = {k: getattr(env, k).clone() for k in FIELDS}
    s.update({k: getattr(env.state, k).clone() for k in STATE})
    return s


def restore(env, s):
    for k in FIELDS:
        getattr(env, k).copy_(s[k])
    for k in STATE:
        getattr(env.state, k).copy_(s[k])


def make_env(torch, monkeypatch, kernel, n):
    from isaacgym_amd.tensor_api import TAEnv
    monkeypatch.setenv("PPENV_TA_KERNEL", kernel)
    env = TAEnv(n, device=DEV, seed=3, env=dict(episodeLength=L_EP))
    assert env.sim.kernel == kernel and env.fused
    gen = torch.Generator(device=DEV).manual_seed(n)
    acts = torch.rand(3, n, 27, device=DEV, generator=gen) * 2 - 1
    for k in range(2):                                                        # away from the initial pose
        env.step(acts[k])
    return env, acts[2].contiguous()


def prepare_case(torch, env, n, case, rng):
    """Random count and sticky bits in `flags`; progress so that (a) nobody, (b) only env n - 1, (c) everybody resets in the next step."""
    env.state.flags.copy_(torch.from_numpy(B.random_flags(n, rng).astype(np.int32)))
    prog = np.zeros(n, np.int64)
    if case == "b":
        prog[n - 1] = L_EP - 2
    elif case == "c":
        prog[:] = L_EP - 2
    env.state.progress_buf.copy_(torch.from_numpy(prog))
    return snapshot(env)


def preclear_counts(env, start, action):
    """The head-counts right before the clear of the step from `start`: the same step with max_episode_length raised (nobody resets, so
    nothing is cleared) and the struct detached."""
    restore(env, start)
    real = env.params.max_episode_length
    env.params.max_episode_length = B.RAISED
    try:
        env.step(action)
        assert not bool(env.reset_buf.any())
        return B.popcounts(env.state.flags.cpu().numpy().view(np.uint32))
    finally:
        env.params.max_episode_length = real


@pytest.mark.parametrize("n", [1, 63, 64, 130])
@pytest.mark.parametrize("kernel", ["chain", "quad", "lane"])
def test_step_kernels_sum_before_they_clear(torch_cuda, monkeypatch, kernel, n):
    torch = torch_cuda
    env, action = make_env(torch, monkeypatch, kernel, n)
    rng = np.random.default_rng(1000 * n + len(kernel))
    out = env.enable_outcomes()
    assert out.dtype == torch.int64 and out.shape == (16,) and not bool(out.any()) and env.enable_outcomes() is out
    want = np.zeros(B.WORDS, np.uint64)
    for case, resets in (("a", 0), ("b", 1), ("c", n), ("b", 1)):
        start = prepare_case(torch, env, n, case, rng)
        env.sim.set_outcome(out)
        env.step(action)
        with_struct = snapshot(env)
        assert int(env.reset_buf.sum()) == resets
        env.sim.set_outcome(None)
        counts = preclear_counts(env, start, action)
        restore(env, start)
        env.step(action)                                                      # the pointer NULL, the real max_episode_length
        plain = snapshot(env)
        for k in plain:
            assert torch.equal(with_struct[k], plain[k]), f"{kernel}, n {n}, case {case}: {k}"
        if resets:
            B.add_window(want, n, counts)
            assert not bool((plain["flags"] & B.COUNT_MASK).any())
        np.testing.assert_array_equal(words(out), want, err_msg=f"{kernel}, n {n}, case {case}")
    assert int(want[0]) == 3 and int(want[1]) == 3 * n
    f = env.outcome_fields()
    assert int(f["windows"]) == 3 and int(f["last_envs"]) == n and [int(f[k]) for k in ("closer", "hit_paddle", "cross_net", "hit_table", "fall_down")] == want[2:7].tolist()
    env.close()


# -------------------------------------------------------------------------------------------------------------------- 3. a captured step
def test_captured_step_replays_like_an_eager_one(torch_cuda, monkeypatch):
    torch = torch_cuda
    n = 130
    env, action = make_env(torch, monkeypatch, "chain", n)
    out = env.enable_outcomes()
    start = prepare_case(torch, env, n, "c", np.random.default_rng(5))
    env.step(action)
    eager = words(out)
    assert int(eager[0]) == 1 and int(eager[1]) == n and int(eager[2:7].sum()) > 0
    after = snapshot(env)
    restore(env, start)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(action)
    torch.cuda.synchronize()
    assert words(out).tobytes() == eager.tobytes()                            # capturing ran nothing
    out.zero_()
    for _ in range(5):
        restore(env, start)
        g.replay()
    torch.cuda.synchronize()
    got = words(out)
    np.testing.assert_array_equal(got[:7], 5 * eager[:7])
    np.testing.assert_array_equal(got[7:13], eager[7:13])
    for k, v in snapshot(env).items():
        assert torch.equal(v, after[k]), k
    env.close()


# ------------------------------------------------------------------------------------------------------------------- 4. the setter, off
def test_setter_off_stops_the_counting(torch_cuda, monkeypatch):
    torch = torch_cuda
    n = 64
    env, action = make_env(torch, monkeypatch, "chain", n)
    out = env.enable_outcomes()
    rng = np.random.default_rng(6)
    prepare_case(torch, env, n, "c", rng)
    env.step(action)
    one = words(out)
    assert int(one[0]) == 1
    env.sim.set_outcome(None)
    prepare_case(torch, env, n, "c", rng)
    env.step(action)
    assert int(env.reset_buf.sum()) == n and words(out).tobytes() == one.tobytes()
    env.sim.set_outcome(out)
    prepare_case(torch, env, n, "c", rng)
    env.step(action)
    assert int(words(out)[0]) == 2
    with pytest.raises(ValueError):
        env.sim.set_outcome(torch.zeros(16, dtype=torch.int32, device=DEV))
    env.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. the Player
from test_play_gpu import checkpoint, load_policy, make_plain  # noqa: E402,F401  (checkpoint: a module-scoped fixture)


def test_player_outcomes_do_not_depend_on_polling(torch_cuda, checkpoint):
    """130 envs, episodeLength 12: every env resets at control steps 11 and 22, so games_num = 200 is crossed during the second window."""
    from isaacgym_amd.play import Player
    path = checkpoint(TA)
    runs = []
    for poll in (1, 7, 64):
        task = make_plain(TA, 130, 21)
        assert task.outcomes is None and "outcomes" not in task.extras
        pl = Player(task, load_policy(path), games_num=200, poll_every=poll, max_steps=2000, outcomes=True)
        res = pl.run()
        assert task.extras["outcomes"] is task.outcomes is task.env.outcome
        runs.append((res, pl.stats.state_bytes(), words(task.outcomes)))
    o = runs[0][0]["outcomes"]
    assert runs[0][0]["outcomes"] == runs[1][0]["outcomes"] == runs[2][0]["outcomes"]
    assert (o["windows"], o["envs"], o["last_envs"]) == (2, 260, 130)
    names = ("closer", "hit_paddle", "cross_net", "hit_table", "fall_down")
    assert all(o[f"{k}_rate"] == o[k] / 260 and 0 <= o[k] <= 260 and o[f"last_{k}"] <= o[k] for k in names)
    assert runs[0][0]["steps_played"] == 22 and runs[2][0]["steps_played"] == 64
    assert int(runs[2][2][0]) > 2                                              # the live struct went on counting; the latched copy did not
    plain = Player(make_plain(TA, 130, 21), load_policy(path), games_num=200, poll_every=64, max_steps=2000)
    ref = plain.run()
    assert "outcomes" not in ref
    assert plain.stats.state_bytes() == runs[2][1]
    for k in ref:
        if k != "seconds":
            assert ref[k] == runs[2][0][k], k
    # no window before the first reset: the rates are None
    fresh = Player(make_plain(TA, 130, 21), load_policy(path), games_num=200, poll_every=1, max_steps=5, outcomes=True)
    none = fresh.run()["outcomes"]
    assert none["windows"] == 0 and all(none[f"{k}_rate"] is None for k in names)


def test_other_tasks_refuse(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player
    TT = "HumanoidPingpongTiltG1"
    task = make_plain(TT, 64, 21)
    with pytest.raises(ValueError, match="keep no count tensors"):
        task.enable_outcomes()
    with pytest.raises(ValueError, match="keep no count tensors"):
        Player(task, load_policy(checkpoint(TT)), games_num=10, outcomes=True)


# --------------------------------------------------------------------------------------------------------------------- 6. the trainer
def make_trainer(torch, outcomes):
    import isaacgym_amd
    from isaacgym_amd import ppo, scene
    cfg = scene.default_task_cfg("TA")
    cfg["env"]["episodeLength"] = 40                                           # windows at control steps 39 and 78 of the 96 in 3 epochs
    task = isaacgym_amd.make(seed=7, task=TA, num_envs=128, cfg=cfg)
    return ppo.PPOTrainer(task, ppo.PPOConfig(minibatch_size=1024), seed=7, outcomes=outcomes)


def test_trainer_with_outcomes_is_bitwise_the_trainer_without(torch_cuda):
    torch = torch_cuda
    runs = []
    for outcomes in (False, True):
        tr = make_trainer(torch, outcomes)
        results = []
        for e in range(3):
            if e > 0:
                torch.cuda.set_sync_debug_mode("error")                       # still no host read in an epoch
            try:
                results.append(tr.train_epoch())
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        state = [t.clone() for t in tr.learner.parameters() + [tr.logstd] + list(tr.opt.exp_avg) + list(tr.opt.exp_avg_sq) + [tr.opt.state[tr.opt.cur]]]
        for rms in (tr.learner.rms, tr.value_rms):
            assert rms is not None
            state += [rms.running_mean.clone(), rms.running_var.clone(), rms.count.clone(), rms.mean.clone(), rms.inv_std.clone()]
        runs.append((tr, results, state, tr.meter.state_bytes()))
    (_, r0, s0, m0), (tr, r1, s1, m1) = runs
    assert len(s0) == len(s1) and all(torch.equal(a, b) for a, b in zip(s0, s1))
    assert m0 == m1
    for a, b in zip(r0, r1):
        assert set(b) - set(a) == {"outcome_windows", "outcome_envs"} | {f"outcome_{k}" for k in ("closer", "hit_paddle", "cross_net", "hit_table", "fall_down")}
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert [int(r["outcome_windows"]) for r in r1] == [0, 1, 2]
    assert int(r1[0]["outcome_envs"]) == 0 and all(float(r1[0][f"outcome_{k}"]) == 0.0 for k in ("closer", "fall_down"))
    assert int(r1[2]["outcome_envs"]) == 128
    w = words(tr.outcome)
    for i, k in enumerate(("closer", "hit_paddle", "cross_net", "hit_table", "fall_down")):
        v = r1[2][f"outcome_{k}"]
        assert v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda
        assert float(v) == float(np.float32(int(w[8 + i])) / np.float32(128))
    assert "outcome" not in tr.state_dict() and not any("outcome" in k for k in tr.state_dict())


def test_two_ranks_sum_the_last_window(tmp_path):
    import torch
    worker = os.path.join(ROOT, "tests", "ta_outcome_dp_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc_per_node=2", worker, "--out", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    r0, r1 = (torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2))
    assert r0["world"] == r1["world"] == 2
    names = ("closer", "hit_paddle", "cross_net", "hit_table", "fall_down")
    for a, b in zip(r0["results"], r1["results"]):
        for k in ["outcome_windows", "outcome_envs"] + [f"outcome_{n}" for n in names]:
            assert torch.equal(a[k], b[k]), k
    last = r0["results"][-1]
    assert int(last["outcome_windows"]) == 2 and int(last["outcome_envs"]) == 256
    own = [r["own"].numpy().view(np.uint64) for r in (r0, r1)]
    assert [int(o[7]) for o in own] == [128, 128]
    for i, n in enumerate(names):
        assert float(last[f"outcome_{n}"]) == float(np.float32(int(own[0][8 + i] + own[1][8 + i])) / np.float32(256))
