"""The keyed random streams on the device (tests/test_rng_streams_host.py has the contract and the host side): the kernels of two seeds, two
ranks, two families never draw one number twice, and the hardware's Box-Muller is the fp64 one to a measured bound.  A "seed" here is a USER
seed, handed to its owners: every env handle below is the `env` of a TASK made with that seed (make_env), the sampler is driven through
PPOTrainer, RLGamesPolicy.act and policy.sampler_stream_seed, the tables through a task's own reset-randomisation plan."""
import numpy as np
import pytest

import dr_shim_binding as drs
from isaacgym_amd import scene
from test_rng_streams_host import gauss64, rows_of, shared

pytestmark = pytest.mark.gpu

# Largest |device - fp64 Box-Muller| of a unit normal: v_log_f32, v_sqrt_f32, v_sin_f32 / v_cos_f32 and the fp32 product against numpy in double on
# the same uniforms.  Measured on an MI355X: 5.03e-7 over the sampler test's draws (4.40e-7 at 7 actions, 5.02e-7 at 27), 4.32e-7 over the
# observation-noise test's (TT 3.74e-7, T4 4.32e-7, TA 3.95e-7, beyond the rounding of the fp32 add that carries the draw into the observation).
# Asserted: four times the largest — the instructions are deterministic per input, the margin is for inputs these seeds do not visit.
E_MEASURED = 5.03e-7
E = 4 * E_MEASURED


from isaacgym_amd.policy import sampler_stream_seed  # noqa: E402
from test_rng_streams_host import env_seed as env_stream_seed, tables_seed as tables_stream_seed  # noqa: E402  (VecTask.native_seeds)

TASK_NAMES = {"TT": "HumanoidPingpongTiltG1", "T4": "Humanoid12PingpongTiltG1", "TA": "HumanoidPingpongTiltNESSparse27DOFG1"}


def make_env(task, n, seed, env_id_offset=0, episode_length=None):
    """The native handle (PPEnv / TAEnv) of a TASK made with the user seed `seed`, as isaacgym_amd.make() makes it (cfg["seed"],
    cfg["env_id_offset"]: make(multi_gpu=True) sets the latter to rank x num_envs)."""
    from isaacgym_amd.tasks import isaacgym_task_map
    cfg = scene.default_task_cfg(task)
    cfg["env"]["numEnvs"], cfg["seed"], cfg["env_id_offset"] = n, seed, env_id_offset
    if episode_length is not None:
        cfg["env"]["episodeLength"] = episode_length
    t = isaacgym_task_map[TASK_NAMES[task]](cfg, "cuda:0", "cuda:0", -1, True, False, False)
    t.env._task = t            # the task lives as long as its handle is used
    return t.env


# ------------------------------------------------------------------------------------------------------------------- who owns a user seed
def test_tasks_trainer_and_policy_hand_down_stream_seeds(monkeypatch):
    """isaacgym_amd.make(seed) keys its handle by the env stream of the seed (7-dof config, 27-dof params), PPOTrainer(seed) its collector by the
    sampler stream, RLGamesPolicy.act(seed) likewise; and two tasks made with seeds 6 and 7 serve different balls (raw seeds: 64 of 64 the same)."""
    import torch
    import isaacgym_amd
    from isaacgym_amd import ppo
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    n, serves = 64, {}
    for seed in (6, 7):
        t = isaacgym_amd.make(seed=seed, task="HumanoidPingpongTiltG1", num_envs=n)
        assert int(t.native_config.seed) == int(t.env.config.seed) == env_stream_seed(seed)
        t.env.reset_all()
        torch.cuda.synchronize()
        serves[seed] = t.env.ball[7:10].t().cpu().numpy().copy()
        if seed == 6:
            tr = ppo.PPOTrainer(t, ppo.PPOConfig(minibatch_size=32 * n), seed=seed)
            assert tr.seed == seed and tr.col.seed == sampler_stream_seed(seed)
        ta = isaacgym_amd.make(seed=seed, task="HumanoidPingpongTiltNESSparse27DOFG1", num_envs=n)
        assert int(ta.env.params.seed) == env_stream_seed(seed)
    assert shared(serves[6], serves[7]) == 0


def test_stochastic_act_draws_from_the_sampler_stream(tmp_path):
    """RLGamesPolicy.act(deterministic=False, seed=s): bit for bit sample_actions on the network's mu under sampler_stream_seed(s) at the
    policy's counter — and not the draw under s itself, which is the action noise of an env seeded s."""
    import torch
    from isaacgym_amd.policy import RLGamesPolicy, sample_actions
    from test_policy_mlp import _rlgames_state_dict
    gen = torch.Generator().manual_seed(4)
    units, num_obs, num_act, m = (2048, 1536, 1024, 1024, 512, 512), 313, 27, 256
    torch.save({"model": _rlgames_state_dict(torch, num_obs, units, num_act, gen)}, tmp_path / "p.pth")
    pol = RLGamesPolicy.load(str(tmp_path / "p.pth"), "cuda:0")
    obs = (torch.randn(m, num_obs, generator=gen) * 1.5).cuda()
    mu = pol.net.forward(obs)[0].clone()
    for step, seed in enumerate((42, 42, 43), 1):
        got = pol.act(obs, deterministic=False, seed=seed)[0].clone()
        want, raw = torch.zeros_like(got), torch.zeros_like(got)
        sample_actions(want, mu, pol.sigma, sampler_stream_seed(seed), step, -1.0, 1.0)
        sample_actions(raw, mu, pol.sigma, seed, step, -1.0, 1.0)
        assert torch.equal(got, want), (step, seed)
        assert float((got != raw).float().mean()) > 0.9


# ------------------------------------------------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize("a", [7, 27])
def test_sampler_rows_differ_across_seeds_and_counters(a):
    """sample_actions and heads_sample, 256 rows, seeds 42 .. 49 (the eight ranks of a data-parallel run), one counter, unclamped: all 8 x 256
    rows of (raw - mu) / sigma are different draws (under raw seeds: 64 distinct rows), a second counter gives 256 more, heads_sample is still
    heads followed by sample_actions bit for bit, and with mu = 0, sigma = 1 the draw is the fp64 Box-Muller of the sampler's own stream."""
    import torch
    from isaacgym_amd.policy import heads_sample, layer_forward, sample_actions
    m, k = 256, 64
    gen = torch.Generator().manual_seed(a)
    x = (torch.randn(m, k, generator=gen) * 0.5).half().cuda()
    w = (torch.randn(a + 1, k, generator=gen) / 8).half().cuda()
    b = (torch.randn(a + 1, generator=gen) * 0.1).half().cuda()
    sigma = torch.full((a,), 0.5, device="cuda")
    out1, out2 = torch.zeros(m, a + 1, device="cuda"), torch.zeros(m, a + 1, device="cuda")
    layer_forward(out1, x, w, b, elu=False)
    mu = out1[:, :a]
    g_rows = []
    for seed, counter in [(s, 5) for s in range(42, 50)] + [(42, 6)]:
        act1, act2 = torch.zeros(m, a, device="cuda"), torch.zeros(m, a, device="cuda")
        nl1, nl2 = torch.zeros(m, device="cuda"), torch.zeros(m, device="cuda")
        sample_actions(act1, mu, sigma, sampler_stream_seed(seed), counter, 0.0, 0.0, nl1)
        heads_sample(out2, x, w, b, a, act2, sigma, sampler_stream_seed(seed), counter, 0.0, 0.0, nl2)
        assert torch.equal(out1, out2) and torch.equal(act1, act2) and torch.equal(nl1, nl2), (seed, counter)
        g_rows.append(((act1.double() - mu.double()) / 0.5).cpu().numpy())
    allg = np.concatenate(g_rows)
    assert np.isfinite(allg).all() and len(rows_of(allg)) == 9 * m
    # the stream itself: mu = 0, sigma = 1 -> raw is g
    zero, one, raw = torch.zeros(m, a, device="cuda"), torch.ones(a, device="cuda"), torch.zeros(m, a, device="cuda")
    worst = 0.0
    for seed in (42, 43):
        sample_actions(raw, zero, one, sampler_stream_seed(seed), (3 << 24) + 5, 0.0, 0.0)  # counter's high part keys as the episode
        ref = gauss64(sampler_stream_seed(seed), np.arange(m)[:, None], 3, 5, np.arange(a)[None, :])
        worst = max(worst, float(np.abs(raw.cpu().numpy().astype(np.float64) - ref).max()))
    print(f"sampler [a={a}]: largest |device - fp64| = {worst:.3e} of a unit normal")
    assert worst <= E


# ------------------------------------------------------------------------------------------------------------------- serves
def _ppenv_serves(variant, n, seed, env_id_offset=0):
    """[n, 6]: the ball velocity of two consecutive episodes — after reset_all, then after reset_idx of every env"""
    import torch
    env = make_env(variant, n, seed, env_id_offset)
    assert int(env.config.seed) == env_stream_seed(seed) and env.config.env_id_offset == env_id_offset
    env.reset_all()
    v0 = env.ball[7:10].t().clone()
    env.reset_idx(torch.arange(n))
    v1 = env.ball[7:10].t().clone()
    torch.cuda.synchronize()
    assert int(env.episode.min()) == int(env.episode.max()) and env.status == 0
    out = torch.cat([v0, v1], 1).cpu().numpy()
    env.close()
    return out


def _ta_serves(n, seed):
    """[n, 15]: ball y, z and velocity of three consecutive episodes of the 27-dof task — at creation, after reset_idx of every env, and after a
    step in which every env times out (the kernel's own draw)."""
    import torch
    env = make_env("TA", n, seed, episode_length=30)
    assert int(env.params.seed) == env_stream_seed(seed)
    take = lambda: torch.cat([env.root_states[:, 2, 1:3], env.root_states[:, 2, 7:10]], 1).clone()
    s0 = take()
    env.reset_idx()
    s1 = take()
    env.state.progress_buf.fill_(28)
    env.step(torch.zeros(n, 27, device="cuda"))
    torch.cuda.synchronize()
    assert int(env.reset_buf.sum()) == n and int(env.state.episode.min()) == 2 and env.sim.status == 0
    s2 = take()
    want = scene.ta_reset_draws(env.params, torch.arange(n), torch.full((n,), 2)).numpy()
    np.testing.assert_allclose(s2.cpu().numpy()[:, :2], want[:, :2], rtol=0, atol=1e-6)    # y, z: one fp32 product and sum of the draw
    np.testing.assert_allclose(s2.cpu().numpy()[:, 2:], want[:, 2:], rtol=0, atol=1e-4)    # the serve: fp32 sines on the device, double on the host
    out = torch.cat([s0, s1, s2], 1).cpu().numpy()
    env.close()
    return out


@pytest.mark.parametrize("n", [64, 130])
@pytest.mark.parametrize("task", ["TT", "T4", "TA"])
def test_serves_of_neighbouring_seeds_are_different_serves(task, n, monkeypatch):
    """For seeds (6, 7) and (42, 43): no env's serves of consecutive episodes under one seed are an env's under the other (n = 130: a ragged last
    workgroup).  Under raw seeds the 7-dof tasks served 64 of 64 (130 of 130: 128) envs the balls of the other seed, permuted."""
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    serves = (lambda s: _ta_serves(n, s)) if task == "TA" else (lambda s: _ppenv_serves(task, n, s))
    for a, b in [(6, 7), (42, 43)]:
        assert shared(serves(a), serves(b)) == 0, (a, b)


def test_shards_of_two_ranks_and_of_one_seed():
    """Ranks 0 and 1 of a data-parallel run, (63, offset 0) and (64, offset 64) at n = 64, serve disjoint balls (raw seeds: 64 of 64 shared); two
    shards under a COMMON seed are still the n = 128 handle bit for bit."""
    r0, r1 = _ppenv_serves("TT", 64, 63, 0), _ppenv_serves("TT", 64, 64, 64)
    assert shared(r0, r1) == 0
    whole = _ppenv_serves("TT", 128, 63, 0)
    np.testing.assert_array_equal(np.concatenate([r0, _ppenv_serves("TT", 64, 63, 64)]).view(np.uint32), whole.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- tables
def test_tables_of_neighbouring_seeds_share_no_column():
    """n = 64, seeds 23 and 22.  A TT task in "reset" mode with the yaml's randomisation block: the plan it uploads carries the tables' stream
    of its seed, and no env's column of its tables under one seed is a column under the other (raw seeds: 64 of 64); the same for a
    ResetRandomizer on the mixed plan under the seeds the tasks derive (all 23 table rows); the device is the host build of the kernel
    body bit for bit everywhere."""
    import torch
    from isaacgym_amd import _lib
    from isaacgym_amd.dr import ResetRandomizer
    from isaacgym_amd.env import PPEnv
    from test_dr_reset_gpu import make_task
    n, plan, cols, tcols = 64, drs.mixed_plan(frequency=1), {}, {}
    ones = torch.ones(n, dtype=torch.int64, device="cuda")
    for seed in (23, 22):
        task = make_task(TASK_NAMES["TT"], n, seed, drs.task_block(TASK_NAMES["TT"]), frequency=1, apply_at="reset")
        rr = task.env.reset_randomization
        host = drs.HostDR(rr.plan, n, seed=tables_stream_seed(seed))
        for _ in range(2):
            rr.apply(ones)
            host.apply(np.ones(n, np.int64))
        torch.cuda.synchronize()
        dev = {k: v.cpu().numpy().reshape(-1, n) for k, v in rr.tables.items()}
        for k in dev:
            np.testing.assert_array_equal(dev[k].view(np.uint32), host.tables[k].view(np.uint32), err_msg=f"task, {k}, seed {seed}")
        tcols[seed] = np.ascontiguousarray(np.concatenate([dev[k] for k in sorted(dev)]).T)
        rr = ResetRandomizer(_lib.lib(), "cuda:0", n, plan, PPEnv.DR_TABLE_ROWS, seed=tables_stream_seed(seed))
        host = drs.HostDR(plan, n, seed=tables_stream_seed(seed))
        for _ in range(2):
            rr.apply(ones)
            host.apply(np.ones(n, np.int64))
        torch.cuda.synchronize()
        dev = {k: v.cpu().numpy().reshape(-1, n) for k, v in rr.tables.items()}
        for k in dev:
            np.testing.assert_array_equal(dev[k].view(np.uint32), host.tables[k].view(np.uint32), err_msg=f"{k}, seed {seed}")
        cols[seed] = np.ascontiguousarray(np.concatenate([dev[k] for k in sorted(dev)]).T)
    assert cols[23].shape == (n, 23) and shared(cols[23], cols[22]) == 0
    assert tcols[23].shape[1] >= 7 and shared(tcols[23], tcols[22]) == 0


# ------------------------------------------------------------------------------------------------------------------- observation noise
SIGMA = 64.0           # a power of two: sigma x g is exact, and (noisy - clean) / 64 recovers g to the rounding of one fp32 add


def _noise_handles(task, n, seed):
    """Two handles (of two tasks made with the user seed) in one state with unit tables, observation noise 0 and SIGMA -> (clean, noisy, read): read() = (episode [n], progress [n])"""
    import torch
    ones = lambda *shape: torch.ones(*shape, device="cuda")
    if task == "TA":
        from test_ta_physics import load_chain_state
        envs = [make_env("TA", n, seed) for _ in range(2)]
        c = envs[0]
        load_chain_state(envs[1], c.root_states.cpu().numpy(), c.dof_states.cpu().numpy(), c.state.flags.cpu().numpy().view(np.uint32),
                         c.state.episode.cpu().numpy().view(np.uint32), c.state.progress_buf.cpu().numpy())
        tabs = dict(dof_stiffness_scale=ones(27, n), dof_damping_scale=ones(27, n), link_mass_scale=ones(28, n), restitution_scale=ones(n), friction_scale=ones(n))
        read = lambda: (c.state.episode.cpu().numpy().astype(np.int64), c.state.progress_buf.cpu().numpy())
    else:
        envs = [make_env(task, n, seed) for _ in range(2)]
        c = envs[0]
        c.reset_all()
        torch.cuda.synchronize()
        envs[1].set_state(c.get_state())
        tabs = dict(dof_stiffness_scale=ones(7, n), dof_damping_scale=ones(7, n), link_mass_scale=ones(7, n), restitution_scale=ones(n), friction_scale=ones(n))
        read = lambda: (c.episode.cpu().numpy().astype(np.int64), c.progress_buf.cpu().numpy()[::c.num_agents])
    envs[0].set_randomization(**tabs, observation_noise_sigma=0.0)
    envs[1].set_randomization(**tabs, observation_noise_sigma=SIGMA)
    return envs[0], envs[1], read


def _recovered_noise(task, n, seed, steps=4):
    """-> per step: g [n, columns per env] = (noisy - clean) / SIGMA in double, the rounding bound of its fp32 add, the fp64 reference and the
    identity of the draw behind every element (gauss64)."""
    import torch
    clean, noisy, read = _noise_handles(task, n, seed)
    na = {"TT": 7, "T4": 14, "TA": 27}[task]
    width = {"TT": 80, "T4": 160, "TA": scene.TA_NUM_OBS}[task]               # T4: the env's two agent rows side by side = indices 16 .. 175
    base = 32 if task == "TA" else 16
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        ep, prog = read()
        act = ((torch.rand(clean.obs_buf.shape[0], na if task == "TA" else 7, generator=gen) - 0.5) * 0.6).cuda()
        clean.step(act); noisy.step(act)
        torch.cuda.synchronize()
        oc, on = (e.obs_buf.cpu().numpy().astype(np.float64).reshape(n, width) for e in (clean, noisy))
        ref, ids = gauss64(env_stream_seed(seed), np.arange(n)[:, None], ep[:, None], prog[:, None], base + np.arange(width)[None, :], ta=task == "TA", draw_ids=True)
        out.append(((on - oc) / SIGMA, 2.0 ** -24 * (np.abs(oc) + np.abs(on)) / SIGMA, ref, ids, oc))
    assert clean.status == 0
    clean.close(); noisy.close()
    return out


@pytest.mark.parametrize("task", ["TT", "T4", "TA"])
def test_observation_noise_is_the_keyed_box_muller(task, monkeypatch):
    """The observation noise recovered on the device, n = 64, four steps, seeds 5 and 6: every element is the fp64 Box-Muller of ITS key — the pair
    of its index, cosine branch for an even index and sine for an odd one, under the stream seed, the episode and the progress at the step's start
    — to 2^-24 (|clean| + |noisy|) / 64 (the rounding of the one fp32 add, derived) + E (the hardware's transcendentals, measured: above).

    Distinctness.  An fp32 normal has ~2^24 values where the density is: among the 20 032 draws of one 27-dof step some two hundred million
    pairs exist, and a handful coincide by chance under ANY generator (birthday), so equality of values cannot be the test.  What holds the DEVICE
    to its keys is the elementwise comparison above: each device value is within 2e-6 of the draw of its own key and of no other.  The second
    half checks the key lattice, on the restatement alone: the draws behind all elements of a step, of the next step and of seed + 1 have
    pairwise different identities (u1 bits, u2 bits, branch: 49 bits, chance 1e-6 over all pairs).  A key used twice — within a row, across
    envs, across steps, across seeds — fails one or the other.  As device values, beside it: no two columns (an index over the 64 envs) and no
    two rows (an env over its indices) of a step agree in more than two places, nor any with the next step's or the other seed's.  The 2: two
    unrelated fp32 normals are equal with probability ~3e-8 (density^2 integrated x the 2^-24 grid), so over the at most 313 x 313 x 64 = 6e6
    places compared per pair of steps 0.2 equal places are expected in all, and three in ONE pair of vectors have probability below 1e-15;
    a shared key makes all 64 (or all 80 .. 313) places of a pair equal.

    Pooled moments over n x columns x 4 steps (N): |mean| <= 6 / sqrt N, |var - 1| <= 6 sqrt(2 / N), |kurtosis - 3| <= 6 sqrt(24 / N)."""
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    n = 64
    runs = {seed: _recovered_noise(task, n, seed) for seed in (5, 6)}
    worst, pooled = 0.0, []
    for seed, steps in runs.items():
        for t, (g, rnd, ref, ids, oc) in enumerate(steps):
            live = oc.std(axis=0) > 0                                               # every non-constant column
            assert live.sum() >= 0.75 * live.size, (task, int(live.sum()))
            assert np.isfinite(g).all()
            err = np.abs(g - ref)[:, live] - rnd[:, live]
            worst = max(worst, float(err.max()))
            pooled.append(g[:, live].ravel())
    print(f"observation noise [{task}]: largest |device - fp64| beyond the rounding of the add = {worst:.3e} of a unit normal")
    # identities: within a step, with the next step, with the other seed
    for seed, steps in runs.items():
        for t in range(len(steps)):
            here = steps[t][3].ravel()
            assert np.unique(here).size == here.size, (seed, t)
            if t + 1 < len(steps):
                assert np.intersect1d(here, steps[t + 1][3].ravel()).size == 0, (seed, t)
            assert np.intersect1d(here, np.concatenate([s[3].ravel() for s in runs[11 - seed]])).size == 0, (seed, t)
    # values: columns and rows as vectors
    def agree(a, b):                                                               # [p, d], [q, d] -> the largest number of equal places of a row of a and one of b
        return max(int((a[i][None, :] == b).sum(axis=1).max()) for i in range(len(a)))
    g0, g1, h0 = runs[5][0][0], runs[5][1][0], runs[6][0][0]
    for a, b in ((g0, g1), (g0, h0)):
        assert agree(a, b) <= 2 and agree(a.T, b.T) <= 2
    same = lambda a: max(int((a[i][None, :] == a[i + 1:]).sum(axis=1).max()) for i in range(len(a) - 1))
    assert same(g0) <= 2 and same(np.ascontiguousarray(g0.T)) <= 2
    x = np.concatenate(pooled)
    N, mean, var = x.size, x.mean(), x.var()
    kurt = ((x - mean) ** 4).mean() / var ** 2
    print(f"observation noise [{task}]: N = {N}, mean {mean:+.4f}, var {var:.4f}, kurtosis {kurt:.4f}")
    assert abs(mean) <= 6 / np.sqrt(N) and abs(var - 1) <= 6 * np.sqrt(2.0 / N) and abs(kurt - 3) <= 6 * np.sqrt(24.0 / N)
    assert worst <= E, worst
