"""The cases of tests/test_step_hybrid_schedule_gpu.py, checked on the oracle alone before a GPU sees them (tests/step_schedule_scenarios.py):
the oracle's own sensitivity probe sets aside at most 2 % of every case's env-steps, and in every case the ball's path depends on the arm's
geometry — what the step kernels' waves hand to each other."""
import pytest

import step_schedule_scenarios as ss


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_every_case_stays_under_the_probe_cap_and_reaches_the_arm(oracle_lib, variant):
    for v, n, substeps, dr in ss.CASES:
        if v != variant:
            continue
        r = ss.oracle_run(v, n, substeps, dr)
        what = f"[{v}, n={n}, substeps={substeps}{', randomised' if dr else ''}, seed {ss.seed_of(v, n, substeps, dr)}]"
        assert r.cfg.substeps == substeps and len(r.steps) == ss.STEPS
        assert r.excluded <= ss.EXCLUDED_CAP * n * ss.STEPS, f"{what}: the probe sets aside {r.excluded} of {n * ss.STEPS} env-steps"
        assert r.arm_contacts >= ss.min_arm_contacts(n), f"{what}: only {r.arm_contacts} env-steps depend on the arm's geometry"


def test_the_cases_are_the_ones_the_schedule_can_get_wrong():
    assert set(n for _, n, _, _ in ss.CASES) == {1, 63, 65, 130} and set(s for _, _, s, _ in ss.CASES) == {1, 2, 3, 4}
    assert set(v for v, _, _, _ in ss.CASES) == {"TT", "TN", "T3"} and set(dr for _, _, _, dr in ss.CASES) == {False, True}
    assert len(ss.CASES) == len(set(ss.CASES)) == 96
