"""Reset-time domain randomisation (apply_at: "reset") as the 27-dof and the 4-actor steps see it: parity with the oracle under the tables
a task drew on the device, a redraw reaching exactly its env's next step, the seed and env id offset of a task reaching the plan, a
captured step + redraw pair replaying like eager ones, and clear_randomization giving the plain kernel back.  The 7-dof task rides
along where a property was pinned for no family.  Every bound is the one of the test named next to it; the rest is bitwise.
Need a real MI355X."""
import numpy as np
import pytest

import dr_shim_binding as drs
from helpers import ExclusionLog, SensitivityProbe, mask_envs, obs_atol, reward_atol
from isaacgym_amd import scene
from test_dr_reset_gpu import TABLES, bits, make_task

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def block_of(name):
    """The golden yaml block of the task (the 4-actor variant has no yaml of its own in the reference: it runs the 3-actor block)."""
    return drs.task_block(TT if name == T4 else name)


def step_tables(env):
    """The five tensors whose addresses the step kernel holds."""
    return env.dr_tables


def table_bits(rr):
    n = rr.num_envs
    return {k: bits(rr.tables[k]).reshape(-1, n).copy() for k in TABLES}


def changed_columns(now, before):
    """-> {table: bool [N]}, which columns differ in any row."""
    return {k: np.any(now[k] != before[k], axis=0) for k in TABLES}


def snapshot(env):
    """Every tensor a step reads or writes, env-major [N, ...] as raw 32 / 64-bit words: {name: array}.  The two agent rows of a 4-actor
    env sit side by side in its row."""
    n = env.num_envs
    raw = lambda t: (lambda a: a.view(np.uint32) if a.dtype == np.float32 else a)(t.detach().cpu().numpy())
    if hasattr(env, "sim"):          # TAEnv
        d = dict(root=env.root_states, dof=env.dof_states, dof_force=env.dof_force_tensor, flags=env.state.flags, episode=env.state.episode,
                 progress=env.progress_buf, obs=env.obs_buf, rew=env.rew_buf, reset=env.reset_buf)
        return {k: raw(v).reshape(n, -1) for k, v in d.items()}
    soa = dict(dof_pos=env.dof_pos, dof_vel=env.dof_vel, dof_force=env.dof_force, ball=env.ball, flags=env.flags, episode=env.episode)
    out = {k: raw(v).reshape(-1, n).T.copy() for k, v in soa.items()}
    out.update({k: raw(v).reshape(n, -1) for k, v in dict(progress=env.progress_buf, obs=env.obs_buf, rew=env.rew_buf, reset=env.reset_buf).items()})
    return out


DOF_KEYS = ("dof", "dof_pos", "dof_vel")


def copy_state(src, dst):
    """src's state into dst: get_state / set_state for PPEnv; root, dof, flags, episode and progress for TAEnv (test_ta_physics's load)."""
    if hasattr(src, "sim"):
        for a, b in ((src.root_states, dst.root_states), (src.dof_states, dst.dof_states), (src.state.flags, dst.state.flags),
                     (src.state.episode, dst.state.episode), (src.state.progress_buf, dst.state.progress_buf)):
            b.copy_(a)
    else:
        dst.set_state(src.get_state())


def uploaded_plan(torch, rr):
    """The ppenv_dr_plan the kernels read, back from device memory."""
    torch.cuda.synchronize()
    return scene.DRPlan.from_buffer_copy(rr.plan_dev.cpu().numpy().tobytes())


# ------------------------------------------------------------------------------------- 1. parity under the drawn tables, 27-dof
def test_27dof_step_under_the_drawn_tables_matches_oracle(torch_cuda, oracle_lib, monkeypatch):
    """60 task steps in "reset" mode (episodeLength 33: every env times out once, at step 33, and redraws), then the five tables are read
    back and given to the oracle exactly as test_ta_chain_kernel_with_randomisation_matches_oracle gives it host-made tables — its loop,
    tolerances, sensitivity mask, ta_chain_check_excluded and bound 0.005 (test_ta_physics.run_chain_dr_step_parity) — together with the
    yaml's noise amplitudes and one gravity.  12 steps, each restarted from the oracle's tensors, starting from the mid-episode state the
    rollout left (progress 27: every env times out again inside them, so the reset path runs under the drawn tables too).  The oracle
    alone, under tables of this distribution (tests/dr_shim_binding.HostDR) and states of its own rollout, sets aside 0 of 7680
    env-steps."""
    from test_ta_physics import run_chain_dr_step_parity
    torch = torch_cuda
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    n = 640
    block = block_of(TA)
    task = make_task(TA, n, 31, block, env={"episodeLength": 33}, frequency=5, apply_at="reset")
    env, rr = task.env, task.env.reset_randomization
    assert env.sim.kernel == "chain" and task._dr_reset
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    for _ in range(60):
        task.step(torch.rand(n, 27, device="cuda:0", generator=gen) * 2 - 1)
    assert int(rr.draws.sum()) > n + 30
    tabs = {k: rr.tables[k].cpu().numpy().copy() for k in TABLES}
    assert all(np.ptp(v) > 1e-3 for v in tabs.values())                              # every table is in play
    kw = dict(action_noise_sigma=float(block["actions"]["range"][1]), observation_noise_sigma=float(block["observations"]["range"][1]))
    gz = float(scene.TA_GRAVITY_Z) - 0.3
    env.set_noise_sigmas(**kw)
    env.set_gravity(gz)
    assert all(env.sim._dr[i] is rr.tables[k] for i, k in enumerate(TABLES))         # the step still reads the tensors the kernel rewrites
    env.materialize_rb = True                                                        # the comparison reads the step's rigid_body_states
    cfg, m = scene.build_ta_scene(n), scene.build_ta_model()
    cfg.gravity_z = gz
    torch.cuda.synchronize()
    state = [env.root_states.cpu().numpy().copy(), env.dof_states.cpu().numpy().copy(), env.state.flags.cpu().numpy().view(np.uint32).copy(),
             env.state.episode.cpu().numpy().view(np.uint32).copy(), env.progress_buf.cpu().numpy().copy()]
    assert state[4].min() > 0 and (state[3] == 1).all()                              # mid-episode, one reset behind every env
    resets, _ = run_chain_dr_step_parity(oracle_lib, env, cfg, m, tabs, kw, f"gpu 27-dof chain-wave step under device-drawn tables vs oracle [n={n}]",
                                         12, state, np.random.default_rng(21))
    assert resets >= n
    for k in TABLES:                                                                 # env.step alone does not redraw
        np.testing.assert_array_equal(rr.tables[k].cpu().numpy(), tabs[k], err_msg=k)
    assert env.sim.status == 0


# ------------------------------------------------------------------------------------- 2. parity under the drawn tables, 4-actor
def test_4actor_step_under_the_drawn_tables_matches_oracle(torch_cuda, oracle_lib):
    """120 task steps in "reset" mode, then 8 compared steps as test_t4_fused_step_with_randomisation_matches_oracle runs them
    (OracleEnv.set_randomization(**tabs, **kw), SensitivityProbe, _check_step, its tolerances and bound 0.01), from the mid-episode state
    the rollout left.  The oracle applies an env's [7][N] column to both humanoids: its dof rows 0-6 and 7-13 and both observation rows
    are compared, so both agent rows were stepped under that column; and a second handle given the same numbers as host tables
    (the path that test pins) steps bit for bit like the one reading the device-drawn tensors.  During the rollout the rule runs beside
    it on the host (HostDR, reset_rows 2: row 2 e decides) from the task's own reset_buf: the tables end bit-identical.  The oracle alone,
    under such tables and its own rollout's states, sets aside 4 of 2048 env-steps (0.2 %)."""
    from isaacgym_amd.env import PPEnv
    from test_t4_fused import DevView, _check_step
    torch = torch_cuda
    n = 256
    block = block_of(T4)
    task = make_task(T4, n, 17, block, frequency=5, apply_at="reset")
    env, rr, cfg = task.env, task.env.reset_randomization, task.native_config
    assert rr.reset_rows == 2 and env.num_agents == 2
    host = drs.HostDR(rr.plan, n, seed=scene.stream_seed(17, scene.STREAM_TABLES), env_id_offset=0, reset_rows=2)   # the task's seed as its plan gets it
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    for _ in range(120):
        task.step(torch.rand(2 * n, 7, device="cuda:0", generator=gen) * 2 - 1)
        reset = task.reset_buf.cpu().numpy()
        assert (reset[0::2] == reset[1::2]).all()
        host.apply(reset)
    assert int(rr.draws.sum()) > n + 30
    np.testing.assert_array_equal(rr.draws.cpu().numpy(), host.draws)
    tabs = {k: rr.tables[k].cpu().numpy().copy() for k in TABLES}
    for k in TABLES:
        np.testing.assert_array_equal(tabs[k].reshape(-1).view(np.uint32), host.tables[k].reshape(-1).view(np.uint32), err_msg=k)
    assert all(np.ptp(v) > 1e-3 for v in tabs.values())
    kw = dict(action_noise_sigma=float(block["actions"]["range"][1]), observation_noise_sigma=float(block["observations"]["range"][1]))
    o = oracle_lib.OracleEnv(cfg, threads=8)
    probe = SensitivityProbe(oracle_lib, cfg)
    ref = PPEnv(type(cfg).from_buffer_copy(cfg), device="cuda:0")
    ref.set_randomization(**{k: torch.from_numpy(v) for k, v in tabs.items()}, **kw)
    for x in (o, probe.o2):
        x.set_randomization(**tabs, **kw)
    for x in (o, probe.o2, env, ref):
        x.set_gravity(-9.8 - 0.3)
    env.set_noise_sigmas(**kw)
    assert all(env._dr[i] is rr.tables[k] for i, k in enumerate(TABLES))             # the step still reads the tensors the kernel rewrites
    torch.cuda.synchronize()
    o.set_state(env.get_state())                                                     # a mid-episode state, 120 steps in
    oa, ra = obs_atol() + 2e-6, 2 * reward_atol(cfg)
    log = ExclusionLog("gpu 4-actor step under device-drawn tables vs oracle", bound=0.01)
    rng = np.random.default_rng(8)
    for t in range(8):
        actions = rng.uniform(-1.2, 1.2, (2 * n, 7)).astype(np.float32)
        st = o.get_state()
        env.set_state(st)
        ref.set_state(st)
        o.step(actions)
        a = torch.from_numpy(actions).cuda()
        env.step(a)
        ref.step(a)
        keep = ~probe.sensitive(st, actions, o)
        log.add(keep)
        g = DevView(env)
        probe.check_excluded(log, t, st, actions, o, g, keep, oa, ra)
        _check_step(mask_envs(g, keep, 2), mask_envs(o, keep, 2), t, oa, ra)
        for name in ("obs_buf", "rew_buf", "reset_buf", "dof_pos", "dof_vel", "dof_force", "ball", "flags"):
            assert torch.equal(getattr(env, name), getattr(ref, name)), (name, t)
    log.close()
    for k in TABLES:                                                                 # env.step alone does not redraw
        np.testing.assert_array_equal(rr.tables[k].cpu().numpy(), tabs[k], err_msg=k)
    assert env.status == 0
    ref.close()


# ------------------------------------------------------------------------- 3. a redraw reaches the next step, for that env only
@pytest.mark.parametrize("name", [TT, TA, T4])
def test_redraw_takes_effect_on_the_next_step_for_that_env_only(torch_cuda, monkeypatch, name):
    """Two identical handles A and B (n = 130: two full step workgroups and a ragged one of two envs), tables drawn by one all-ones
    application, three steps under scripted reset buffers — the last lists envs 1, 65 and 127 through their row `reset_rows * e` (and,
    for the 4-actor variant, the second agent row alone of envs 2 and 66, which must not count): exactly those redraw, in both handles.
    Then A alone redraws ids = [0, 63, 64, 128, 129] (apply_reset_randomization(ids), the reset_idx path) and, with no synchronisation
    of the test's in between, both step on one action tensor.  Bitwise: every env outside ids is equal in every tensor of the step —
    the neighbours of a redrawn env in its workgroup included, whose table rows share an LDS tile with it on the 27-dof task — every
    env in ids differs in its dof state (per agent row for the 4-actor variant), and A's columns differ from B's at ids and nowhere
    else.  27-dof: its count-flag clear couples the envs of a launch when any resets (TA:1162-1166); four steps into 160-step episodes
    with no early stop none does, and reset_buf is asserted all zero."""
    torch = torch_cuda
    if name == TA:
        monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    n, freq = 130, 3
    ids = [0, 63, 64, 128, 129]
    listed = np.isin(np.arange(n), ids)
    A, B = (make_task(name, n, 9, block_of(name), frequency=freq, apply_at="reset") for _ in range(2))
    ea, eb = A.env, B.env
    ra, rb = ea.reset_randomization, eb.reset_randomization
    rows, R, na = n * ea.num_agents, ea.num_agents, A.num_actions
    assert ra.reset_rows == R
    ones = torch.ones(rows, dtype=torch.int64, device="cuda:0")
    for e, r in ((ea, ra), (eb, rb)):
        r.apply(ones)
        e.set_noise_sigmas(action_noise_sigma=0.02, observation_noise_sigma=0.002)
        assert all(step_tables(e)[i] is r.tables[k] for i, k in enumerate(TABLES))
    copy_state(ea, eb)
    first = table_bits(ra)
    assert all(len(np.unique(v)) > n // 2 for v in first.values())                   # non-trivial tables
    script = np.zeros((freq, rows), np.int64)
    due = np.isin(np.arange(n), [1, 65, 127])
    script[freq - 1, R * np.flatnonzero(due)] = 1
    if R == 2:
        script[freq - 1, [2 * 2 + 1, 2 * 66 + 1]] = 1                                # the second agent's row alone does not decide
    gen = torch.Generator(device="cuda:0").manual_seed(4)
    for t in range(freq):
        a = torch.rand(rows, na, device="cuda:0", generator=gen) * 2 - 1
        row = torch.from_numpy(script[t]).cuda()
        for e, r in ((ea, ra), (eb, rb)):
            e.step(a)
            r.apply(row)
    for r in (ra, rb):
        np.testing.assert_array_equal(r.randomize_buf.cpu().numpy(), np.where(due, 0, freq))
        for k, c in changed_columns(table_bits(r), first).items():
            np.testing.assert_array_equal(c, due, err_msg=f"{k}: columns the scripted resets rewrote")
    before = table_bits(rb)
    for k in TABLES:
        np.testing.assert_array_equal(table_bits(ra)[k], before[k], err_msg=k)
    for k, v in snapshot(ea).items():
        np.testing.assert_array_equal(v, snapshot(eb)[k], err_msg=f"{k} before the redraw")
    a = torch.rand(rows, na, device="cuda:0", generator=gen) * 2 - 1
    ids_dev = torch.tensor(ids, device="cuda:0")
    torch.cuda.synchronize()
    ea.apply_reset_randomization(ids_dev)                                            # A only; nothing below waits for it
    ea.step(a)
    eb.step(a)
    sa, sb = snapshot(ea), snapshot(eb)
    dof_differs = np.zeros((n, R), bool)
    for k in sa:
        same = (sa[k] == sb[k]).reshape(n, -1).all(axis=1)
        assert same[~listed].all(), (k, np.flatnonzero(~same & ~listed)[:8])
        if k in DOF_KEYS:
            dof_differs |= (sa[k] != sb[k]).reshape(n, R, -1).any(axis=2)            # [N, R]: the SoA dof rows are agent-major, 7 per agent
    assert dof_differs[listed].all(), dof_differs[listed]
    if name == TA:
        assert all((sa[k][1:63] == sb[k][1:63]).all() for k in sa)                   # the redrawn envs' neighbours in workgroup 0
        assert not sa["reset"].any() and not sb["reset"].any()
    if R == 2:
        obs_differs = (sa["obs"] != sb["obs"]).reshape(n, 2, -1).any(axis=2)
        assert obs_differs[listed].all() and not obs_differs[~listed].any()
    now = table_bits(ra)
    for k, c in changed_columns(now, before).items():
        np.testing.assert_array_equal(c, listed, err_msg=f"{k}: A's columns against B's")
    for k, c in changed_columns(table_bits(rb), before).items():
        assert not c.any(), k
    np.testing.assert_array_equal(ra.draws.cpu().numpy(), 1 + due + listed)
    np.testing.assert_array_equal(ra.randomize_buf.cpu().numpy(), np.where(due | listed, 0, freq))
    np.testing.assert_array_equal(rb.draws.cpu().numpy(), 1 + due)
    assert ea.status == 0


# --------------------------------------------------------------------------------------------- 4. task-level shard invariance
@pytest.mark.parametrize("name", [TT, T4])
def test_two_task_shards_compute_the_whole_task(torch_cuda, name):
    """One task of 256 envs and two of 128 with cfg["env_id_offset"] 0 and 128, the same cfg["seed"], "reset" mode, frequency 3, the
    golden block with its noise, gravity and schedules, driven for 80 task.step calls with the halves of one action stream; resets are
    the tasks' own (episodeLength 48 adds a time-out to the early stops, so that every env resets inside the run).  After every step
    the halves' tables, randomize_buf, draws, obs_buf, rew_buf and reset_buf, concatenated, are the whole's bit for bit.
    The 27-dof task is left out: its count-flag clear (TA:1162-1166) reads every env of the launch — when any env of the launch resets,
    the count flags of ALL its envs are cleared — so a half and the whole are not the same computation; its plumbing is pinned by
    test_27dof_task_hands_its_seed_and_offset_to_the_plan."""
    torch = torch_cuda
    n, h = 256, 128
    block = block_of(name)
    kw = dict(env={"episodeLength": 48}, frequency=3, apply_at="reset")
    whole = make_task(name, n, 5, block, **kw)
    halves = [make_task(name, h, 5, block, env_id_offset=off, **kw) for off in (0, h)]
    R = whole.num_agents
    for t, off in zip(halves, (0, h)):
        P = uploaded_plan(torch, t.env.reset_randomization)
        assert (P.seed, P.env_id_offset, P.num_envs, P.reset_rows, P.frequency) == (scene.stream_seed(5, scene.STREAM_TABLES), off, h, R, 3)     # the tables' stream of the task's seed
    gen = torch.Generator(device="cuda:0").manual_seed(6)
    cat = lambda f, axis=0: np.concatenate([f(t) for t in halves], axis=axis)
    redraws_after_first = 0
    for step in range(80):
        a = torch.rand(n * R, 7, device="cuda:0", generator=gen) * 2 - 1
        whole.step(a)
        halves[0].step(a[: h * R])
        halves[1].step(a[h * R:])
        rw = whole.env.reset_randomization
        for k in TABLES:
            np.testing.assert_array_equal(cat(lambda t: bits(t.env.reset_randomization.tables[k]).reshape(-1, h), axis=1), bits(rw.tables[k]).reshape(-1, n),
                                          err_msg=f"{k}, step {step}")
        np.testing.assert_array_equal(cat(lambda t: t.randomize_buf.cpu().numpy()), whole.randomize_buf.cpu().numpy(), err_msg=f"randomize_buf, step {step}")
        np.testing.assert_array_equal(cat(lambda t: t.env.reset_randomization.draws.cpu().numpy()), rw.draws.cpu().numpy(), err_msg=f"draws, step {step}")
        for buf in ("obs_buf", "rew_buf", "reset_buf"):
            np.testing.assert_array_equal(cat(lambda t: bits(getattr(t, buf)) if buf != "reset_buf" else t.reset_buf.cpu().numpy()),
                                          bits(getattr(whole, buf)) if buf != "reset_buf" else whole.reset_buf.cpu().numpy(), err_msg=f"{buf}, step {step}")
    redraws_after_first = int(whole.env.reset_randomization.draws.sum()) - n
    assert redraws_after_first >= 30, redraws_after_first
    assert bool((halves[1].env.reset_randomization.tables["link_mass_scale"] != halves[0].env.reset_randomization.tables["link_mass_scale"]).any())


def test_27dof_task_hands_its_seed_and_offset_to_the_plan(torch_cuda, monkeypatch):
    """The plumbing half of the shard property for the 27-dof task (see test_two_task_shards_compute_the_whole_task for why only this):
    cfg["seed"] and cfg["env_id_offset"] reach task.env.params and the plan the kernel reads, and after the first task.step — whose
    application redraws every env — a 128-env task at offset 128 holds, bit for bit, the tables the kernel body gives on the CPU
    (HostDR(plan, 128, seed, env_id_offset=128)) for one all-ones application."""
    torch = torch_cuda
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    n, seed, off = 128, 21, 128
    task = make_task(TA, n, seed, block_of(TA), env_id_offset=off, frequency=3, apply_at="reset")
    rr, p = task.env.reset_randomization, task.env.params
    tseed = scene.stream_seed(seed, scene.STREAM_TABLES)                           # the task hands each family its own stream of cfg["seed"]
    assert (int(p.seed), int(p.env_id_offset)) == (scene.stream_seed(seed, scene.STREAM_ENV), off)
    P = uploaded_plan(torch, rr)
    assert (P.seed, P.env_id_offset, P.num_envs, P.reset_rows, P.frequency) == (tseed, off, n, 1, 3)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    task.step(torch.rand(n, 27, device="cuda:0", generator=gen) * 2 - 1)
    host = drs.HostDR(rr.plan, n, seed=tseed, env_id_offset=off)
    host.apply(np.ones(n, np.int64))
    for k in TABLES:
        np.testing.assert_array_equal(bits(rr.tables[k]), host.tables[k].reshape(-1).view(np.uint32), err_msg=k)
    assert bool((rr.draws == 1).all()) and not bool(task.randomize_buf.any())
    unshifted = drs.HostDR(rr.plan, n, seed=tseed, env_id_offset=0)
    unshifted.apply(np.ones(n, np.int64))
    assert (unshifted.tables["link_mass_scale"] != host.tables["link_mass_scale"]).any()   # the offset is in the numbers


# ------------------------------------------------------------------------------------------------------------ 5. graph replay
@pytest.mark.parametrize("name", [TT, TA])
def test_captured_step_and_redraw_replay_like_eager_ones(torch_cuda, monkeypatch, name):
    """One env.step + apply_reset_randomization pair captured with torch.cuda.graph (one stream, no parallel branches, a static action
    buffer) and replayed 40 times, beside a twin task that runs 40 eager pairs on the same actions: tables, randomize_buf, draws, every
    state tensor, obs_buf and reset_buf are bitwise equal at the end — the redraw of step t is ordered before step t + 1 by the stream
    alone.  The env-level pair is captured, not VecTask.step: its host-side apply_randomizations reads the gravity draw with .item(),
    a synchronisation no capture admits.  n = 130; episodeLength 12 makes every env reset (and, at frequency 3, redraw) three times."""
    torch = torch_cuda
    if name == TA:
        monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    n, K = 130, 40
    G, E = (make_task(name, n, 13, block_of(name), env={"episodeLength": 12}, frequency=3, apply_at="reset") for _ in range(2))
    eg, ee = G.env, E.env
    rg, re_ = eg.reset_randomization, ee.reset_randomization
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    acts = torch.rand(K + 2, n, G.num_actions, device="cuda:0", generator=gen) * 2 - 1
    for k in range(2):                                                               # warm-up: code objects loaded, first application done
        for e in (eg, ee):
            e.step(acts[k])
            e.apply_reset_randomization()
    static = acts[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eg.step(static)
        eg.apply_reset_randomization()
    torch.cuda.synchronize()
    assert torch.equal(rg.steps, re_.steps) and torch.equal(rg.draws, re_.draws)     # capturing ran nothing
    for k in range(2, K + 2):
        static.copy_(acts[k])
        g.replay()
        ee.step(acts[k])
        ee.apply_reset_randomization()
    torch.cuda.synchronize()
    tg, te = table_bits(rg), table_bits(re_)
    for k in TABLES:
        np.testing.assert_array_equal(tg[k], te[k], err_msg=k)
    for attr in ("randomize_buf", "draws", "steps"):
        assert torch.equal(getattr(rg, attr), getattr(re_, attr)), attr
    sg, se = snapshot(eg), snapshot(ee)
    for k in sg:
        np.testing.assert_array_equal(sg[k], se[k], err_msg=k)
    assert bool((re_.steps == K + 2).all())
    assert int(re_.draws.sum()) - n >= n, int(re_.draws.sum())
    assert all(len(np.unique(v)) > n // 2 for v in te.values())


# ------------------------------------------------------------------------------------------------ 6. clearing after "reset" mode
@pytest.mark.parametrize("name", [TA, T4])
def test_clear_after_reset_mode_gives_the_plain_kernel_back(torch_cuda, monkeypatch, name):
    """clear_randomization() after "reset" mode: reset_randomization is None, apply_reset_randomization refuses, and the next steps are
    the plain kernel's bit for bit (a task created without randomisation, from the same state).  The handle is driven at the env level,
    so the task's gravity randomisation — which clear_randomization does not own — never ran."""
    from isaacgym_amd import _lib
    from isaacgym_amd.tasks import isaacgym_task_map
    torch = torch_cuda
    if name == TA:
        monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    n = 130
    task = make_task(name, n, 7, block_of(name), frequency=3, apply_at="reset")
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[name])
    cfg["env"]["numEnvs"], cfg["seed"] = n, 7
    plain = isaacgym_task_map[name](cfg, "cuda:0", "cuda:0", -1, True, False, False)
    env, pe = task.env, plain.env
    rows = n * task.num_agents
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    env.set_noise_sigmas(action_noise_sigma=0.02, observation_noise_sigma=0.002)
    for _ in range(5):
        env.step(torch.rand(rows, task.num_actions, device="cuda:0", generator=gen) * 2 - 1)
        env.apply_reset_randomization()
    tables = env.reset_randomization.tables
    assert all(bool((tables[k] != 1.0).any()) for k in TABLES)
    env.clear_randomization()
    assert env.reset_randomization is None and step_tables(env) is None
    with pytest.raises(_lib.PPEnvError, match="no plan"):
        env.apply_reset_randomization()
    torch.cuda.synchronize()
    copy_state(env, pe)
    for _ in range(2):
        a = torch.rand(rows, task.num_actions, device="cuda:0", generator=gen) * 2 - 1
        env.step(a)
        pe.step(a)
    se, sp = snapshot(env), snapshot(pe)
    for k in se:
        np.testing.assert_array_equal(se[k], sp[k], err_msg=k)
