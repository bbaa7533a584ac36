"""The HIP step kernels on every cell of the ball's contact code: the scripted states of tests/ball_contact_scenarios.py through PPEnv,
restarted from the oracle's state each step, against the oracle at the suite's tolerances, the probe's set-aside env-steps through
check_excluded.  TT on both schedules, TN and T3 on the two-wave kernel, T4 on its three-wave kernel, and the randomisation
instantiations (TT split and fused, T4) with restitution_scale in [1.3, 1.6] on the paddle and shape groups, where the restitution_max
clamp binds.  The oracle trajectory is computed once per (variant, randomised) and shared; the cells and the set-aside share it reaches are
asserted by tests/test_ball_contacts_host.py without a GPU (and here again for the randomised trajectories, which only these tests run)."""
import numpy as np
import pytest

import ball_contact_scenarios as sc
from helpers import ExclusionLog
from test_ball_contacts_host import SEED, SIZES
from test_t4_fused import DevView

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


CASES = [("TT", "split", False), ("TT", "fused", False), ("TN", "split", False), ("T3", "split", False), ("T4", "split", False),
         ("TT", "split", True), ("TT", "fused", True), ("T4", "split", True)]


@pytest.mark.parametrize("variant,schedule,dr", CASES, ids=[f"{v}-{s}{'-randomised' if d else ''}" for v, s, d in CASES])
def test_step_kernel_on_every_contact_cell(torch_cuda, oracle_lib, monkeypatch, variant, schedule, dr):
    torch = torch_cuda
    from isaacgym_amd import scene
    from isaacgym_amd.env import PPEnv
    n = SIZES[variant]
    assert n % 64
    monkeypatch.setenv("PPENV_STEP_KERNEL", schedule)
    r = sc.oracle_run(variant, n, SEED, dr)
    if dr:        # the clamp must bind where the scenario says, and the randomised trajectory must hold the floor on the humanoids' cells too
        e = np.float32(r.cfg.paddle_restitution) * r.tables["restitution_scale"]
        hit = np.isin(r.meta["group"], (3, 4, 6, 7))
        assert (e[hit] > r.cfg.restitution_max).all() and (e[~hit] < r.cfg.restitution_max).all()
        kept = sc.cell_counts(r)
        low = {k: v for k, v in kept.items() if v < sc.FLOOR}
        assert not low, f"[{variant}, randomised] cells under the floor of {sc.FLOOR} kept env-steps: {low}"
    env = PPEnv(scene.build_config(variant, num_envs=n, seed=sc.ENV_SEED), device="cuda:0")
    if dr:
        env.set_randomization(**r.tables, **sc.DR_NOISE)
    oa, ra = sc.tolerances(r.cfg, dr)
    log = ExclusionLog(f"gpu step on the scripted ball contacts vs oracle [{variant}, {schedule}{', randomised' if dr else ''}]", bound=sc.EXCLUDED_BOUND)
    for t, s in enumerate(r.steps):
        env.set_state(s["st"])
        env.step(torch.from_numpy(s["act"]).cuda())
        g = DevView(env)
        log.add(s["keep"])
        r.probe.check_excluded(log, t, s["st"], s["act"], s["main"], g, s["keep"], oa, ra)
        sc.compare_step(g, s, t, r.cfg, oa, ra, f"gpu [{variant}, {schedule}]")
    log.close()
    env.close()
