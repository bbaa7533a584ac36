"""The 7-dof step kernels at the shapes their wave hand-offs can get wrong: single steps restarted from the oracle's state, 8 per case, at
the suite's tolerances with the probe's set-aside env-steps through check_excluded (tests/helpers.py).

The cases were drawn up for a hybrid schedule of the two-wave kernel, in which the arm wave sweeps the collision geometry of every substep
boundary but the first and hands it to the ball wave through one LDS slot.  That schedule was measured and not kept (11.58
against 11.27 us per step); what ships is the two-wave kernel whose arm wave hands (q, qd) of every boundary to the ball wave, on packed
fp32 pairs.  The cases guard that hand-off in the same places:
  num_envs 1, 63, 65, 130   a lone lane, a ragged workgroup, a second workgroup of one lane, a second ragged workgroup;
  substeps 1, 2, 3, 4       no handed-over boundary, one, and every LDS slot up to the kernel's last;
  TT, TN, T3                the three reward / reset rules (TN keeps the dof state over a reset, T3 ends the episode behind the paddle);
  plain and randomised      the table-reading instantiation of either kernel;
  split and fused           the two-wave and the one-wave schedule.
In every case the ball is on its way to the moving arm, so the geometry of the later boundaries decides where it goes
(tests/test_step_hybrid_schedule_host.py asserts that, and the 2 % cap on the probe's set-aside env-steps, on the oracle alone).
Every case also checks that step_kernel_name reports the kernel that schedule launches and that the status word stays 0."""
import pytest

import ball_contact_scenarios as sc
import step_schedule_scenarios as ss
from helpers import ExclusionLog
from test_t4_fused import DevView

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def kernel_name(schedule, dr):
    tables = "true" if dr else "false"
    return f"step_kernel_split<pp::ModelG1, 1, 0, 1, {tables}>" if schedule == "split" else f"step_kernel<pp::ModelG1, {tables}>"


@pytest.mark.parametrize("schedule", ["split", "fused"])
@pytest.mark.parametrize("variant,n,substeps,dr", ss.CASES, ids=[f"{v}-n{n}-sub{s}{'-randomised' if d else ''}" for v, n, s, d in ss.CASES])
def test_single_steps_match_the_oracle(torch_cuda, oracle_lib, monkeypatch, variant, n, substeps, dr, schedule):
    torch = torch_cuda
    from isaacgym_amd.env import PPEnv
    monkeypatch.setenv("PPENV_STEP_KERNEL", schedule)
    r = ss.oracle_run(variant, n, substeps, dr)
    assert r.excluded <= ss.EXCLUDED_CAP * n * ss.STEPS          # the cap, from the oracle (the host test's assertion, again where it is used)
    env = PPEnv(ss.case_config(variant, n, substeps), device="cuda:0")
    if dr:
        env.set_randomization(**r.tables, **sc.DR_NOISE)
    assert env.step_kernel_name == kernel_name(schedule, dr)
    oa, ra = sc.tolerances(r.cfg, dr)
    what = f"[{variant}, n={n}, substeps={substeps}, {schedule}{', randomised' if dr else ''}]"
    log = ExclusionLog(f"gpu step on the hand-off cases vs oracle {what}", bound=ss.EXCLUDED_CAP)
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
