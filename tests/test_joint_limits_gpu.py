"""The HIP step kernels on every hard switch of the drive: the scripted states of tests/joint_limit_scenarios.py through PPEnv, restarted from the
oracle's state each step, against the oracle at the suite's tolerances, the probe's set-aside env-steps through check_excluded, and — where a
clamp binds with a margin (joint_limit_scenarios.exact_masks) — the focus joint's q, qd and dof_force bit for bit: float32(limit), 0,
+-float32(vel_limit), +-float32(effort), which play_act counts with >=.

Both schedules (the 4-actor variant has one kernel and ignores the switch: it runs under either value) x TT / TN / T3 / T4 at the counted size,
plain and with per-env kp / kd tables (the table-reading instantiations; the gains move the saturation point), TT at the ragged sizes 1, 63, 65,
130 (compared, not counted), and one case captured into a graph and replayed.  The oracle trajectory is computed once per (variant, size,
randomised) and shared; the floor, the cap and "nobody resets" are asserted on the oracle alone by tests/test_joint_limits_host.py, and here
again where the trajectory is used."""
import numpy as np
import pytest

import ball_contact_scenarios as sc
import joint_limit_scenarios as js
from helpers import ExclusionLog
from test_gpu_parity import DevView, make_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def run_steps(torch, env, r, what, counted):
    oa, ra = sc.tolerances(r.cfg)
    log = ExclusionLog(f"gpu step on the scripted joint limits vs oracle {what}", bound=js.EXCLUDED_CAP)
    exact = dict(dof_pos=0, dof_vel=0, dof_force=0)
    for t, s in enumerate(r.steps):
        env.set_state(s["st"])
        env.step(torch.from_numpy(s["act"]).cuda())
        g = DevView(env)
        log.add(s["keep"])
        r.probe.check_excluded(log, t, s["st"], s["act"], s["main"], g, s["keep"], oa, ra)
        sc.compare_step(g, s, t, r.cfg, oa, ra, f"gpu {what}")
        for k, v in js.assert_exact(g, s, r.meta, f"gpu {what}, step {t}").items():
            exact[k] += v
    log.close()
    assert env.status == 0
    if counted:
        print(f"{what} focus-joint values checked bit for bit: {exact}")
        assert min(exact.values()) >= 7 * 2 * js.FLOOR
    return exact


CASES = [(v, s, dr) for v in js.VARIANTS for s in ("split", "fused") for dr in (False, True)]


@pytest.mark.parametrize("variant,schedule,dr", CASES, ids=[f"{v}-{s}{'-randomised_gains' if d else ''}" for v, s, d in CASES])
def test_step_kernel_on_every_drive_cell(torch_cuda, oracle_lib, monkeypatch, variant, schedule, dr):
    n = js.COUNTED
    assert n % 64
    monkeypatch.setenv("PPENV_STEP_KERNEL", schedule)
    r = js.oracle_run(variant, n, dr)
    what = f"[{variant}, {schedule}{', randomised gains' if dr else ''}, n={n}]"
    js.assert_floor(r, what)
    js.assert_cap(r, what)
    env = make_env(js.case_config(variant, n))
    if dr:
        only, ceases = js.gain_dependence(r)
        assert only >= 1 and ceases >= 1
        env.set_randomization(**r.tables, **js.NO_NOISE)
    if variant != "T4":
        assert ("step_kernel_split" in env.step_kernel_name) == (schedule == "split")
        assert env.step_kernel_name.endswith(", true>" if dr else ", false>")
    run_steps(torch_cuda, env, r, what, True)
    env.close()


@pytest.mark.parametrize("schedule", ["split", "fused"])
@pytest.mark.parametrize("n", js.SIZES)
def test_step_kernel_on_the_ragged_sizes(torch_cuda, oracle_lib, monkeypatch, schedule, n):
    """TT with a lone lane and ragged workgroups: compared, not counted."""
    monkeypatch.setenv("PPENV_STEP_KERNEL", schedule)
    r = js.oracle_run("TT", n, False)
    assert r.resets == 0 and r.excluded <= js.EXCLUDED_CAP * n * js.STEPS
    env = make_env(js.case_config("TT", n))
    run_steps(torch_cuda, env, r, f"[TT, {schedule}, n={n}]", False)
    env.close()


def test_graph_replay_equals_eager_on_the_drive_cells(torch_cuda, oracle_lib):
    """The counted TT run's STEPS steps from its start state (the actions are held, so this is the oracle's own trajectory) captured into one graph
    and replayed: bit for bit the eager steps."""
    torch = torch_cuda
    n = js.COUNTED
    r = js.oracle_run("TT", n, False)
    eager, graphed = make_env(js.case_config("TT", n)), make_env(js.case_config("TT", n))
    act = torch.from_numpy(r.steps[0]["act"]).cuda()
    with torch.no_grad():
        graphed.set_state(r.steps[0]["st"])
        graphed.step(act)                                     # lazy initialisation must not happen inside the capture
        graphed.set_state(r.steps[0]["st"])
        eager.set_state(r.steps[0]["st"])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            for _ in range(js.STEPS):
                graphed.step(act)
        g.replay()
        for _ in range(js.STEPS):
            eager.step(act)
    torch.cuda.synchronize()
    for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "dof_pos", "dof_vel", "dof_force", "ball", "flags", "episode"):
        assert torch.equal(getattr(graphed, name), getattr(eager, name)), name
    assert graphed.status == 0 and eager.status == 0
    np.testing.assert_array_equal(DevView(graphed).progress_buf, r.steps[-1]["main"].progress_buf)
    eager.close(); graphed.close()
