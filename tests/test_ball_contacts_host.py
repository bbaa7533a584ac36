"""The scripted states of tests/ball_contact_scenarios.py: stepped by the oracle alone they reach every cell of the ball's contact code
(contact_resolve / contact_box / contact_capsule / contact_disc and the broad phase of ball_substep, csrc/ppenv_device.h) at least FLOOR
times with at most 2 % of the env-steps set aside; then the kernels' arithmetic on the host (ShimEnv) against the oracle on them.  The
same comparison runs on the HIP kernels in tests/test_ball_contacts_gpu.py."""
import numpy as np
import pytest

import ball_contact_scenarios as sc
import shim_binding as sb
from helpers import ExclusionLog

SEED = 1
SIZES = {"TT": 1001, "TN": 1001, "T3": 1001, "T4": 1503}        # what tests/test_ball_contacts_gpu.py runs: ragged, no multiple of 64


@pytest.fixture(scope="module", params=["TT", "TN", "T3", "T4"])
def run(request, oracle_lib):
    return request.param, sc.oracle_run(request.param, SIZES[request.param], SEED)


def test_every_contact_cell_holds_the_floor(run):
    variant, r = run
    kept, before = sc.cell_counts(r), sc.cell_counts(r, kept=False)
    for name in sc.CELLS[variant]:
        print(f"[{variant}] {name:48s} {kept[name]:5d} kept of {before[name]}")
    low = {k: v for k, v in kept.items() if v < sc.FLOOR}
    assert not low, f"[{variant}] cells under the floor of {sc.FLOOR} kept env-steps: {low}"


def test_set_aside_share_is_under_the_bound(run):
    variant, r = run
    n = SIZES[variant]
    aside = sum(int((~s["keep"]).sum()) for s in r.steps)
    print(f"[{variant}] SensitivityProbe set aside {aside} of {n * sc.STEPS} env-steps ({100 * aside / (n * sc.STEPS):.3f} %)")
    assert aside <= sc.EXCLUDED_BOUND * n * sc.STEPS


def test_no_effect_cells_are_free_flight(run, oracle_lib):
    """In the cells where the specification says nothing happens, classify demands that the counterfactual oracles agree with the main run
    exactly; here, that the step is the free flight: the ball's velocity afterwards is the start's plus gravity (where the env did not reset)."""
    variant, r = run
    cfg = r.cfg
    x = oracle_lib.OracleEnv(cfg)
    checked = 0
    for s in r.steps:
        x.set_state(s["st"])
        want = np.array(x.ball[7:10], np.float64) + np.array([[0.0], [0.0], [float(cfg.gravity_z) * float(cfg.dt)]])
        stays = s["main"].reset_buf.reshape(-1, r.num_agents)[:, 0] == 0
        for name in (c for c in sc.CELLS[variant] if c.replace("h2/", "") in sc.NO_EFFECT):
            m = s["cells"][name] & stays
            checked += int(m.sum())
            np.testing.assert_allclose(s["main"].ball[7:10][:, m], want[:, m], rtol=0, atol=2e-6, err_msg=name)
    x.close()
    assert checked > 100


def test_kernel_arithmetic_on_every_contact_cell(run, oracle_lib):
    """ppenv_device.h compiled for the host (fp32), restarted from the oracle's state each step, against the oracle: the suite's integers, terms
    and tolerances; the probe's set-aside env-steps through check_excluded with none unmatched."""
    variant, r = run
    cfg = r.cfg
    s_env = sb.ShimEnv(cfg)
    oa, ra = sc.tolerances(cfg)
    log = ExclusionLog(f"host shim (kernel arithmetic) on the scripted ball contacts vs oracle [{variant}]", bound=sc.EXCLUDED_BOUND)
    o = oracle_lib.OracleEnv(cfg)
    for t, s in enumerate(r.steps):
        o.set_state(s["st"])
        s_env.copy_state_from(o)
        s_env.step(s["act"])
        log.add(s["keep"])
        r.probe.check_excluded(log, t, s["st"], s["act"], s["main"], s_env, s["keep"], oa, ra)
        sc.compare_step(s_env, s, t, cfg, oa, ra, f"host shim [{variant}]")
    o.close()
    log.close()


@pytest.mark.parametrize("variant", ["TT", "T4"])
def test_randomised_trajectories_hold_the_floor_and_bind_the_clamp(oracle_lib, variant):
    """The oracle trajectories of the randomised GPU cases (tables of ball_contact_scenarios.dr_tables, on every oracle involved): every cell at
    the floor, the set-aside share under the bound, restitution x scale above restitution_max on the paddle and shape groups and below it elsewhere."""
    n = SIZES[variant]
    r = sc.oracle_run(variant, n, SEED, True)
    kept = sc.cell_counts(r)
    low = {k: v for k, v in kept.items() if v < sc.FLOOR}
    assert not low, f"[{variant}, randomised] cells under the floor of {sc.FLOOR} kept env-steps: {low}"
    aside = sum(int((~s["keep"]).sum()) for s in r.steps)
    print(f"[{variant}, randomised] SensitivityProbe set aside {aside} of {n * sc.STEPS} env-steps ({100 * aside / (n * sc.STEPS):.3f} %)")
    assert aside <= sc.EXCLUDED_BOUND * n * sc.STEPS
    e = np.float32(r.cfg.paddle_restitution) * r.tables["restitution_scale"]
    hit = np.isin(r.meta["group"], (3, 4, 6, 7))
    assert (e[hit] > r.cfg.restitution_max).all() and (e[~hit] < r.cfg.restitution_max).all()
    assert all(np.float32(r.cfg.shape[s].restitution) == np.float32(r.cfg.paddle_restitution) for s in range(r.cfg.num_shapes))
