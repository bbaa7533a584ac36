"""Reset-time domain randomisation on the device (include/ppenv_dr.h): the HIP kernel against the host build of its own body, the
rule as a task shows it, parity with the oracle under the tables it drew, shard invariance, graph replay, and the per-step mode left
as it was.  Need a real MI355X."""
import copy

import numpy as np
import pytest

import dr_shim_binding as drs
from helpers import ExclusionLog, SensitivityProbe, assert_close, assert_state_close, mask_envs, obs_atol, reward_atol
from isaacgym_amd import scene

pytestmark = pytest.mark.gpu

F32 = np.float32
TABLES = ["dof_stiffness_scale", "dof_damping_scale", "link_mass_scale", "restitution_scale", "friction_scale"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def ta_plan():
    """The 27-dof task's shapes — [27][N], [27][N], [28][N], [N], [N] — with both distributions and all three schedules."""
    p = drs.mixed_plan(frequency=5)
    for name, rows in (("dof_stiffness_scale", 27), ("dof_damping_scale", 27), ("link_mass_scale", 28)):
        p["tables"][name]["rows"] = rows
    return p


def device_dr(plan, n, seed=0, env_id_offset=0, reset_rows=1):
    from isaacgym_amd import _lib
    from isaacgym_amd.dr import ResetRandomizer
    rows = {k: (t["rows"] if t["rows"] > 1 else 0) for k, t in plan["tables"].items()}
    return ResetRandomizer(_lib.lib(), "cuda:0", n, plan, rows, seed=seed, env_id_offset=env_id_offset, reset_rows=reset_rows)


def bits(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint32)


def assert_same(dev, host, what):
    np.testing.assert_array_equal(dev.randomize_buf.cpu().numpy(), host.randomize_buf, err_msg=f"randomize_buf, {what}")
    np.testing.assert_array_equal(dev.draws.cpu().numpy(), host.draws, err_msg=f"draws, {what}")
    assert (dev.steps.cpu().numpy() == host.count[0]).all(), what                     # every workgroup's copy of the step count
    for k in host.tables:
        np.testing.assert_array_equal(bits(dev.tables[k]), host.tables[k].reshape(-1).view(np.uint32), err_msg=f"table {k}, {what}")


# ------------------------------------------------------------------------------------------------------------ 4. kernel = shim
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
@pytest.mark.parametrize("shape,reset_rows", [("7dof", 1), ("27dof", 1), ("7dof", 2)])
def test_kernel_matches_host_build_of_its_body(torch_cuda, n, shape, reset_rows):
    """ppenv_dr_apply (and one ppenv_dr_apply_ids in the middle) against tests/csrc/dr_shim.cpp for the scripted reset sequence of the
    host tests: tables BIT-identical — Gaussian entries included — integer buffers equal, at every step; wave edges; the two rows per
    env of the 4-actor variant (row 2 e decides; row 2 e + 1 is scripted independently on purpose)."""
    torch = torch_cuda
    plan = drs.mixed_plan(frequency=5) if shape == "7dof" else ta_plan()
    steps = 200
    dev = device_dr(plan, n, seed=23, env_id_offset=100, reset_rows=reset_rows)
    host = drs.HostDR(plan, n, seed=23, env_id_offset=100, reset_rows=reset_rows)
    script = drs.scripted_resets(steps, n * reset_rows)
    reset_dev = torch.zeros(n * reset_rows, dtype=torch.int64, device="cuda:0")
    for t in range(steps):
        reset_dev.copy_(torch.from_numpy(script[t]))
        dev.apply(reset_dev)
        host.apply(script[t])
        if t == 57:
            ids = np.arange(0, n, 3)
            dev.apply_ids(torch.from_numpy(ids).cuda())
            host.apply_ids(ids)
        assert_same(dev, host, f"step {t}")
    assert int(host.draws.sum()) > n * (3 if n >= 63 else 1)
    for k, t in plan["tables"].items():
        if t["operation"] == "scaling" and t["distribution"] == "uniform" and not t["schedule"]:
            v = dev.tables[k]
            assert float(v.min()) >= F32(t["range"][0]) and float(v.max()) <= F32(t["range"][1])


def test_entry_points_refuse_bad_arguments(torch_cuda):
    import ctypes as C

    from isaacgym_amd import _lib
    from isaacgym_amd.dr import ResetRandomizer
    L = _lib.lib()
    dev = device_dr(drs.mixed_plan(), 64)
    bad = scene.build_dr_plan(drs.mixed_plan(frequency=0), {k: v.data_ptr() for k, v in dev.tables.items()}, 64)
    assert L.ppenv_dr_plan_upload(C.byref(bad), dev.plan_dev.data_ptr(), None) == -1 and b"frequency" in L.ppenv_last_error()
    assert L.ppenv_dr_apply(dev.plan_dev.data_ptr(), 64, None, dev.randomize_buf.data_ptr(), dev.state.data_ptr(), None) == -1
    assert L.ppenv_dr_apply_ids(dev.plan_dev.data_ptr(), 64, None, 3, dev.randomize_buf.data_ptr(), dev.state.data_ptr(), None) == -1
    assert L.ppenv_dr_state_bytes(0) == 0 and L.ppenv_dr_state_bytes(257) == 2 * 8 + 257 * 4 and L.ppenv_dr_state_draws_offset(257) == 16
    with pytest.raises(ValueError, match="rows"):
        ResetRandomizer(L, "cuda:0", 64, ta_plan(), {k: 7 for k in TABLES})


# ------------------------------------------------------------------------------------------------ 5. the property that matters
def make_task(name, n, seed, block, env_id_offset=0, env=None, **task_over):
    """env: cfg["env"] keys to override (episodeLength); task_over: keys of randomization_params to override."""
    from isaacgym_amd.tasks import isaacgym_task_map
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[name])
    cfg["env"]["numEnvs"], cfg["seed"], cfg["env_id_offset"] = n, seed, env_id_offset
    cfg["env"].update(env or {})
    cfg["task"] = dict(randomize=True, randomization_params=dict(copy.deepcopy(block), **task_over))
    return isaacgym_task_map[name](cfg, "cuda:0", "cuda:0", -1, True, False, False)


def blend_bounds(t, step):
    """The yaml range of a scaling, carried through the schedule blend of the step it was drawn at: v -> v * s + (1 - s) is monotone in
    v in float32 (rounding is monotone), so a draw inside [lo, hi] lands inside [blend(lo), blend(hi)] EXACTLY — and that interval is
    the yaml range itself once the schedule has run out (s = 1).  (The bare yaml range cannot be asserted while s < 1: upstream blends
    a scaling towards 1, and restitution's range (0, 0.7) does not contain 1.)"""
    s = F32(min(step, t["schedule_steps"]) / float(t["schedule_steps"])) if t["schedule"] == "linear" else F32(1.0)
    f = lambda v: F32(F32(F32(v) * s) + F32(F32(1.0) - s))
    return f(t["range"][0]), f(t["range"][1])


@pytest.mark.parametrize("name,n,steps", [("HumanoidPingpongTiltG1", 512, 160), ("HumanoidPingpongTiltNESSparse27DOFG1", 512, 200),
                                          ("Humanoid12PingpongTiltG1", 256, 160)])
def test_columns_change_only_when_their_env_resets(torch_cuda, name, n, steps):
    """A task with the golden yaml block, apply_at "reset", frequency 5, random actions: a column of any table differs from its previous
    value ONLY at a step where that env reported a reset and its randomize_buf had reached `frequency` (and at the first step, where
    upstream redraws every env) — and it does differ then; randomize_buf follows the reference's arithmetic (+= 1 per step, TT:1025;
    0 for exactly the envs that redraw); every scaling stays inside its yaml range as the schedule blends it (blend_bounds).  (The
    4-actor variant, which has no yaml of its own in the reference, runs the 3-actor block: both agent rows of an env reset together.)"""
    torch = torch_cuda
    block = drs.task_block(name if name != "Humanoid12PingpongTiltG1" else "HumanoidPingpongTiltG1")
    task = make_task(name, n, 4, block, frequency=5, apply_at="reset")
    rr = task.env.reset_randomization
    assert task._dr_reset and task.randomize_buf is rr.randomize_buf and task.randomize_buf.dtype == torch.int64 and tuple(task.randomize_buf.shape) == (n,)
    A = task.num_agents
    expect_rows = {"dof_stiffness_scale": getattr(task, "DR_DOF_ROWS", 7), "dof_damping_scale": getattr(task, "DR_DOF_ROWS", 7),
                   "link_mass_scale": getattr(task, "DR_MASS_ROWS", 7), "restitution_scale": 1, "friction_scale": 1}
    assert {k: (v.shape[0] if v.dim() == 2 else 1) for k, v in rr.tables.items()} == expect_rows
    for v in rr.tables.values():
        assert bool((v == 1.0).all())                       # scalings start neutral
    gen = torch.Generator(device="cuda:0").manual_seed(12)
    rbuf, drawn_at = np.zeros(n, np.int64), np.zeros(n, np.int64)
    prev = {k: bits(v).reshape(-1, n).copy() for k, v in rr.tables.items()}
    resets = redraws_after_first = 0
    plan = rr.plan["tables"]
    for t in range(1, steps + 1):
        a = torch.rand(n * A, task.num_actions, device="cuda:0", generator=gen) * 2 - 1
        task.step(a)
        reset = task.reset_buf.cpu().numpy().reshape(n, A)
        assert (reset[:, 0] == reset[:, -1]).all()
        reset = reset[:, 0]
        rbuf += 1
        mask = np.ones(n, bool) if t == 1 else (reset != 0) & (rbuf >= 5)
        rbuf[mask] = 0
        drawn_at[mask] = t
        resets += int((reset != 0).sum())
        redraws_after_first += int(mask.sum()) if t > 1 else 0
        np.testing.assert_array_equal(task.randomize_buf.cpu().numpy(), rbuf, err_msg=f"randomize_buf, step {t}")
        changed = np.zeros(n, bool)
        for k, v in rr.tables.items():
            now = bits(v).reshape(-1, n)
            changed |= np.any(now != prev[k], axis=0)
            prev[k] = now.copy()
        np.testing.assert_array_equal(changed, mask, err_msg=f"columns rewritten, step {t}")
    print(f"{name}: {resets} resets, {redraws_after_first} redraws after the first application, in {steps} steps of {n} envs")
    assert resets > 30 and redraws_after_first > 30, (resets, redraws_after_first)
    assert int(rr.draws.sum()) == n + redraws_after_first
    for k, v in rr.tables.items():
        tab = v.cpu().numpy().reshape(-1, n)
        for e in range(n):
            lo, hi = blend_bounds(plan[k], int(drawn_at[e]))
            assert (tab[:, e] >= lo).all() and (tab[:, e] <= hi).all(), (k, e, drawn_at[e], lo, hi, tab[:, e])
    assert getattr(task.env, "status", 0) == 0


def test_reset_idx_redraws_the_listed_envs(torch_cuda):
    """VecTask.reset_idx(env_ids) -> _reset_idx -> apply_randomizations (TT:809-812, 849-850): the listed envs whose randomize_buf has
    reached `frequency` redraw, nobody else."""
    torch = torch_cuda
    n = 256
    task = make_task("HumanoidPingpongTiltG1", n, 6, drs.task_block("HumanoidPingpongTiltG1"), frequency=3, apply_at="reset")
    rr = task.env.reset_randomization
    a = torch.zeros(n, 7, device="cuda:0")
    for _ in range(4):
        task.step(a)
    before, rb, draws = bits(rr.tables["link_mass_scale"]).reshape(7, n).copy(), task.randomize_buf.cpu().numpy().copy(), rr.draws.cpu().numpy().copy()
    ids = torch.tensor([5, 9, 9, 200], device="cuda:0")
    task.reset_idx(ids)
    due = np.isin(np.arange(n), [5, 9, 200]) & (rb >= 3)
    assert due.any()
    changed = np.any(bits(rr.tables["link_mass_scale"]).reshape(7, n) != before, axis=0)
    np.testing.assert_array_equal(changed, due)
    np.testing.assert_array_equal(task.randomize_buf.cpu().numpy(), np.where(due, 0, rb))
    np.testing.assert_array_equal(rr.draws.cpu().numpy(), draws + due)


# --------------------------------------------------------------------------------------------- 6. parity with the tables it drew
def test_step_under_the_drawn_tables_matches_oracle(torch_cuda, oracle_lib):
    """After 120 task steps in "reset" mode, the tables are read back and given to the oracle (OracleEnv.set_randomization, as
    test_gpu_parity.py::test_randomized_step_matches_oracle does) together with the yaml's noise amplitudes and one gravity; then
    further steps, each restarted from the oracle's state, are compared under the suite's tolerances and sensitivity probe."""
    from test_gpu_parity import DevView
    torch = torch_cuda
    n = 768
    block = drs.task_block("HumanoidPingpongTiltG1")
    task = make_task("HumanoidPingpongTiltG1", n, 17, block, frequency=5, apply_at="reset")
    rr = task.env.reset_randomization
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    for _ in range(120):
        task.step(torch.rand(n, 7, device="cuda:0", generator=gen) * 2 - 1)
    assert int(rr.draws.sum()) > n + 30
    env, cfg = task.env, task.native_config
    tabs = {k: v.cpu().numpy().copy() for k, v in rr.tables.items()}
    assert all(np.ptp(v) > 1e-3 for v in tabs.values())                              # every table is in play
    kw = dict(action_noise_sigma=float(block["actions"]["range"][1]), observation_noise_sigma=float(block["observations"]["range"][1]))
    o = oracle_lib.OracleEnv(cfg, threads=8)
    probe = SensitivityProbe(oracle_lib, cfg)
    for x in (o, probe.o2):
        x.set_randomization(**tabs, **kw)
        x.set_gravity(-9.8 - 0.3)
    env.set_noise_sigmas(**kw)
    env.set_gravity(-9.8 - 0.3)
    assert all(a is b for a, b in zip(env._dr, (rr.tables[k] for k in TABLES)))     # the step still reads the tensors the kernel rewrites
    torch.cuda.synchronize()
    o.set_state(env.get_state())                                                     # a mid-episode state, 120 steps in
    oa, ra = obs_atol() + 2e-6, reward_atol(cfg)
    log = ExclusionLog("gpu step under device-drawn tables vs oracle [TT]", bound=0.01)
    rng = np.random.default_rng(8)
    for t in range(6):
        actions = rng.uniform(-1.2, 1.2, (n, 7)).astype(np.float32)
        st = o.get_state()
        env.set_state(st)
        o.step(actions)
        env.step(torch.from_numpy(actions).cuda())
        keep = ~probe.sensitive(st, actions, o)
        log.add(keep)
        g = DevView(env)
        probe.check_excluded(log, t, st, actions, o, g, keep, oa, ra)
        v, om = mask_envs(g, keep), mask_envs(o, keep)
        np.testing.assert_array_equal(v.reset_buf, om.reset_buf, err_msg=f"reset step {t}")
        np.testing.assert_array_equal(v.flags, om.flags, err_msg=f"flags step {t}")
        assert_state_close(v, om, f"step {t}")
        assert_close(v.obs_buf, om.obs_buf, f"obs step {t}", atol=oa)
        assert_close(v.rew_buf, om.rew_buf, f"rew step {t}", atol=ra)
    log.close()
    for k, v in rr.tables.items():                                                   # env.step alone does not redraw
        np.testing.assert_array_equal(v.cpu().numpy(), tabs[k])


# ------------------------------------------------------------------------------------------------------------ 7. shard invariance
def test_two_shards_draw_the_tables_of_the_whole(torch_cuda):
    """Two 2048-env handles with env_id_offset 0 and 2048, driven with the two halves of one reset script (the upper half launched
    first), hold bit for bit the tables, draws and randomize_buf of one 4096-env handle driven with the whole script."""
    torch = torch_cuda
    plan, steps = drs.mixed_plan(frequency=4), 120
    whole = device_dr(plan, 4096, seed=9)
    halves = [device_dr(plan, 2048, seed=9, env_id_offset=off) for off in (0, 2048)]
    script = drs.scripted_resets(steps, 4096, p=0.15)
    for t in range(steps):
        row = torch.from_numpy(script[t]).cuda()
        whole.apply(row)
        for h, part in zip(halves[::-1], (row[2048:].contiguous(), row[:2048].contiguous())):
            h.apply(part)
    assert int(whole.draws.sum()) > 4096 * 3
    for k in plan["tables"]:
        w = bits(whole.tables[k]).reshape(-1, 4096)
        np.testing.assert_array_equal(np.concatenate([bits(h.tables[k]).reshape(-1, 2048) for h in halves], axis=1), w, err_msg=k)
    np.testing.assert_array_equal(np.concatenate([h.draws.cpu().numpy() for h in halves]), whole.draws.cpu().numpy())
    np.testing.assert_array_equal(np.concatenate([h.randomize_buf.cpu().numpy() for h in halves]), whole.randomize_buf.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ 8. graph replay
def test_captured_launch_replays_like_eager_launches(torch_cuda):
    """One apply launch captured with torch.cuda.graph (one stream, no branches) and replayed K times equals K eager launches bit for
    bit — the step count the linear schedules read, the first-application flag and draws[] live in device memory and are advanced by
    the kernel.  Capture succeeding is also the proof that the launch does not synchronise."""
    torch = torch_cuda
    n, K = 1000, 48
    plan = drs.mixed_plan(frequency=2)
    device_dr(plan, n).apply(torch.ones(n, dtype=torch.int64, device="cuda:0"))      # the code object is loaded before the capture
    eager, replayed = device_dr(plan, n, seed=5), device_dr(plan, n, seed=5)
    script = drs.scripted_resets(K, n, p=0.3)
    r_eager, r_graph = (torch.zeros(n, dtype=torch.int64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        replayed.apply(r_graph)
    torch.cuda.synchronize()
    assert int(replayed.steps.sum()) == 0 and int(replayed.draws.sum()) == 0          # capturing ran nothing
    for k in range(K):
        row = torch.from_numpy(script[k]).cuda()
        r_eager.copy_(row)
        eager.apply(r_eager)
        r_graph.copy_(row)
        g.replay()
    torch.cuda.synchronize()
    assert int(eager.draws.sum()) > n * 4 and bool((eager.steps == K).all())
    for k in plan["tables"]:
        np.testing.assert_array_equal(bits(replayed.tables[k]), bits(eager.tables[k]), err_msg=k)
    for name in ("draws", "steps", "randomize_buf"):
        assert torch.equal(getattr(replayed, name), getattr(eager, name)), name


# ------------------------------------------------------------------------------------------------------------ 9. nothing else moved
@pytest.mark.parametrize("name", ["HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1"])
def test_default_mode_is_the_per_step_host_redraw(torch_cuda, name):
    """randomize: True without an apply_at key: the tables after 12 steps are those of a restatement, written here, of the per-step
    apply_randomizations (every env redrawn on the host every `frequency` control steps, from torch.Generator(seed + 7919), in its
    draw order), bit for bit; no device plan exists and randomize_buf stays zero."""
    torch = torch_cuda
    n, seed, freq = 256, 3, 5
    block = drs.task_block(name)
    task = make_task(name, n, seed, block, frequency=freq)
    assert task.randomize_apply_at == "step" and not task._dr_reset and getattr(task.env, "reset_randomization", None) is None
    dof_rows, mass_rows = getattr(task, "DR_DOF_ROWS", 7), getattr(task, "DR_MASS_ROWS", 7)
    gen = torch.Generator(device="cuda:0").manual_seed(seed + 7919)
    hum = block["actor_params"]["humanoid"]

    def sample(p, shape, last_step):
        a, b = float(p["range"][0]), float(p["range"][1])
        if p["distribution"] == "gaussian":
            v = torch.randn(shape, device="cuda:0", generator=gen) * b + a
        else:
            v = torch.rand(shape, device="cuda:0", generator=gen) * (b - a) + a
        s = min(max(last_step, 0), int(p["schedule_steps"])) / float(p["schedule_steps"]) if p.get("schedule") == "linear" else 1.0
        return v * s + (1.0 - s) if p["operation"] == "scaling" else v * s

    a = torch.zeros(n, task.num_actions, device="cuda:0")
    first, last_step, last_rand, want = True, -1, -1, None
    for t in range(12):
        if first or last_step - last_rand >= freq:
            first, last_rand = False, last_step
            sample(block["sim_params"]["gravity"], (1,), last_step)
            want = [None] * 5
            want[2] = sample(hum["rigid_body_properties"]["mass"], (mass_rows, n), last_step)
            want[4] = sample(hum["rigid_shape_properties"]["friction"], (n,), last_step)
            want[3] = sample(hum["rigid_shape_properties"]["restitution"], (n,), last_step)
            want[0] = sample(hum["dof_properties"]["stiffness"], (dof_rows, n), last_step)
            want[1] = sample(hum["dof_properties"]["damping"], (dof_rows, n), last_step)
        task.step(a)
        last_step = t + 1
    dr = task.env.dr_tables
    for got, w in zip(dr, want):
        assert torch.equal(got, w)
    assert not bool(task.randomize_buf.any())
