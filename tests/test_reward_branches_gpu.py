"""The HIP step kernels on every cell of the reward and reset decision: the scripted states of tests/reward_branch_scenarios.py through PPEnv,
restarted from the oracle's state each step, against the oracle: rew_buf per actor within reward_atol, reset_buf, progress_buf, the flag word per
actor and episode exactly, the observation row and the state (after a reset the whole re-initialised state) at the suite's tolerances; the
env-steps that near_threshold and SensitivityProbe set aside go through check_excluded.  TT on both schedules, TN and T3 on the two-wave kernel, T4
on its three-wave kernel, each in the plain pass and in the reset pass (3 envs in 7 time out in the step their case is aimed at), and TT's reset pass
once more captured into a graph and replayed.  The oracle trajectory is computed once per (variant, pass) and shared; the cells and the set-aside
share it reaches are asserted without a GPU by tests/test_reward_branches_host.py."""
import numpy as np
import pytest

import ball_contact_scenarios as sc
import reward_branch_scenarios as rs
from helpers import ExclusionLog
from test_gpu_parity import DevView, make_env
from test_reward_branches_host import SEED, SIZES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


CASES = [(v, s, r) for v, s in (("TT", "split"), ("TT", "fused"), ("TN", "split"), ("T3", "split"), ("T4", "split")) for r in (False, True)]


@pytest.mark.parametrize("variant,schedule,resets", CASES, ids=[f"{v}-{s}-{'reset_pass' if r else 'plain_pass'}" for v, s, r in CASES])
def test_step_kernel_on_every_reward_cell(torch_cuda, oracle_lib, monkeypatch, variant, schedule, resets):
    torch = torch_cuda
    from isaacgym_amd import scene
    n = SIZES[variant]
    assert n % 64
    monkeypatch.setenv("PPENV_STEP_KERNEL", schedule)
    r = rs.oracle_run(variant, n, SEED, resets)
    env = make_env(scene.build_config(variant, num_envs=n, seed=rs.ENV_SEED))
    if variant != "T4":
        assert ("step_kernel_split" in env.step_kernel_name) == (schedule == "split")
    oa, ra = rs.tolerances(r.cfg)
    what = f"[{variant}, {schedule}, {'reset' if resets else 'plain'} pass]"
    log = ExclusionLog(f"gpu step on the scripted reward branches vs oracle {what}", bound=rs.EXCLUDED_BOUND)
    for t, s in enumerate(r.steps):
        env.set_state(s["st"])
        env.step(torch.from_numpy(s["act"]).cuda())
        g = DevView(env)
        log.add(s["keep"])
        r.probe.check_excluded(log, t, s["st"], s["act"], s["main"], g, s["keep"], oa, ra)
        sc.compare_step(g, s, t, r.cfg, oa, ra, f"gpu {what}")
    log.close()
    assert env.status == 0
    env.close()


def test_graph_replay_equals_eager_on_the_reward_cells(torch_cuda, oracle_lib, monkeypatch):
    """TT's reset pass, its STEPS steps from the start state (the actions are held, so this is the oracle's own trajectory) captured into one graph and
    replayed: bit for bit the eager steps, time-outs, deaths and re-serves included; and on the envs that no step set aside, the oracle's progress,
    episode and flag words at the end."""
    torch = torch_cuda
    from isaacgym_amd import scene
    monkeypatch.setenv("PPENV_STEP_KERNEL", "split")
    n = SIZES["TT"]
    r = rs.oracle_run("TT", n, SEED, True)
    eager, graphed = (make_env(scene.build_config("TT", num_envs=n, seed=rs.ENV_SEED)) for _ in range(2))
    act = torch.from_numpy(r.steps[0]["act"]).cuda()
    with torch.no_grad():
        graphed.set_state(r.steps[0]["st"])
        graphed.step(act)                                     # lazy initialisation must not happen inside the capture
        graphed.set_state(r.steps[0]["st"])
        eager.set_state(r.steps[0]["st"])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            for _ in range(rs.STEPS):
                graphed.step(act)
        g.replay()
        for _ in range(rs.STEPS):
            eager.step(act)
    torch.cuda.synchronize()
    for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "dof_pos", "dof_vel", "dof_force", "ball", "flags", "episode"):
        assert torch.equal(getattr(graphed, name), getattr(eager, name)), name
    assert graphed.status == 0 and eager.status == 0
    keep = np.all([s["keep"] for s in r.steps], axis=0)
    got, want = DevView(graphed), r.steps[-1]["main"]
    assert want.episode[keep].any()
    for name in ("progress_buf", "episode", "flags", "reset_buf"):
        np.testing.assert_array_equal(getattr(got, name)[keep], getattr(want, name)[keep], err_msg=name)
    eager.close(); graphed.close()
