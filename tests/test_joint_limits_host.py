"""The scripted states of tests/joint_limit_scenarios.py, stepped by the oracle alone: every joint takes both stops in the first and in the later
substep, stays on them and leaves them, exceeds its speed cap, saturates its drive before the solve and in the reported dof_force, and has its
action clamped — each at least FLOOR kept env-steps per (joint, cell, sign), with at most 2 % of a run's env-steps set aside and nobody resetting;
then the kernels' arithmetic on the host (ShimEnv: csrc/ppenv_device.h compiled for the CPU) against the oracle on them, at the suite's
tolerances and, where a clamp binds with a margin, bit for bit.  The same comparison runs on the HIP kernels in tests/test_joint_limits_gpu.py."""
import numpy as np
import pytest

import ball_contact_scenarios as sc
import joint_limit_scenarios as js
import shim_binding as sb
from helpers import RTOL, SCALES, ExclusionLog

RUNS = [(v, dr) for v in js.VARIANTS for dr in (False, True)]           # what tests/test_joint_limits_gpu.py counts


@pytest.fixture(scope="module", params=RUNS, ids=[f"{v}{'-randomised_gains' if dr else ''}" for v, dr in RUNS])
def run(request, oracle_lib):
    variant, dr = request.param
    return variant, dr, js.oracle_run(variant, js.COUNTED, dr)


def test_counted_size_is_ragged_and_whole_cycles():
    assert js.COUNTED % 64 and js.COUNTED % (7 * 2 * js.CYCLE) == 0 and not any(n % 64 == 0 for n in js.SIZES)


def test_every_cell_holds_the_floor_under_the_cap_and_nobody_resets(run):
    variant, dr, r = run
    what = f"[{variant}{', randomised gains' if dr else ''}, n={js.COUNTED}, seed {js.seed_of(variant, js.COUNTED, dr)}]"
    assert len(r.steps) == js.STEPS and r.cfg.substeps == 2
    js.assert_floor(r, what)
    js.assert_cap(r, what)
    for s in r.steps:
        assert not s["main"].reset_buf.any() and (s["main"].progress_buf == s["before"].progress_buf + 1).all()
        lo, hi = (np.tile(np.array([getattr(r.cfg.joint[j], k) for j in range(7)], np.float32), r.num_agents)[:, None] for k in ("lower", "upper"))
        assert ((s["before"].dof_pos >= lo) & (s["before"].dof_pos <= hi)).all(), "a start state outside [lower, upper]"


def _differs(a, b, name, row, factor):
    x, y = (getattr(v, name)[row, np.arange(len(row))].astype(np.float64) for v in (a, b))
    return np.abs(x - y) > factor * (RTOL * SCALES[name] + RTOL * np.abs(y))


def test_every_cell_is_reached(run):
    """Recomputed here from what oracle_run kept of the oracles' runs: every kept env-step of a cell differs from its counterfactual by REACHED x the
    comparison tolerance in the focus joint's tensors; on_stop/held ends with q == limit and qd == 0; on_stop/leaves ends off the stop."""
    variant, dr, r = run
    row, joint, env = r.meta["row"], r.meta["joint"], np.arange(js.COUNTED)
    which = {"stop/substep0": ("limits", ("dof_pos", "dof_vel")), "stop/later": ("limits", ("dof_pos", "dof_vel")), "speed_cap": ("vel_limit", ("dof_pos", "dof_vel")),
             "torque/solve": ("effort", ("dof_pos", "dof_vel")), "torque/reported": ("effort", ("dof_force",)), "action_clip": ("clip", ("dof_pos", "dof_vel", "dof_force"))}
    for s in r.steps:
        for sign in js.SIGNS:
            L = np.array([getattr(r.cfg.joint[j], sign) for j in joint], np.float32)
            for cell, (cf, names) in which.items():
                m = s["cells"][f"{cell}/{sign}"] & s["keep"]
                assert np.any([_differs(s["cf"][cf], s["main"], name, row, js.REACHED) for name in names], axis=0)[m].all(), (cell, sign)
            m = s["cells"][f"on_stop/held/{sign}"]
            assert (s["before"].dof_pos[row, env][m] == L[m]).all() and (s["before"].dof_vel[row, env][m] == 0).all()
            assert (s["main"].dof_pos[row, env][m] == L[m]).all() and (s["main"].dof_vel[row, env][m] == 0).all()
            m = s["cells"][f"on_stop/leaves/{sign}"]
            assert (s["before"].dof_pos[row, env][m] == L[m]).all() and (s["main"].dof_pos[row, env][m] != L[m]).all()
            assert ((s["main"].dof_pos[row, env][m] - L[m]) * (1 if sign == "lower" else -1) > 0).all()        # inside the range
            m = s["cells"][f"torque/reported/{sign}"]
            eff = np.array([r.cfg.joint[j].effort for j in joint], np.float32) * np.float32(1 if sign == "upper" else -1)
            assert (s["main"].dof_force[row, env][m] == eff[m]).all()


def test_the_drawn_substep_is_the_one_substep_oracles(run):
    """A stop drawn for substep 0 (the distance a fraction < 1 of the first substep's travel) is taken by the one-substep oracle, one drawn for the
    later substep (fraction > 1) is not and is taken by the end of the step: in step 0, for every env of the stop shares, kept or not."""
    variant, dr, r = run
    s, kind, sign = r.steps[0], r.meta["kind"], r.meta["sign"]
    for name in js.SIGNS:
        mine = sign == (1.0 if name == "upper" else -1.0)
        for cell, other in (("stop/substep0", "stop/later"), ("stop/later", "stop/substep0")):
            drawn = (kind == cell) & mine
            assert ((r.meta["fraction"][drawn] < 1.0) == (cell == "stop/substep0")).all()
            assert s["cells"][f"{cell}/{name}"][drawn].all() and not s["cells"][f"{other}/{name}"][drawn].any(), (cell, name)


@pytest.mark.parametrize("variant", js.VARIANTS)
def test_randomised_gains_move_the_saturation_point(oracle_lib, variant):
    """From the tables: some env-steps saturate the focus drive only because of the env's gain scale, and some cease to."""
    r = js.oracle_run(variant, js.COUNTED, True)
    only, ceases = js.gain_dependence(r)
    print(f"[{variant}] env-steps whose focus drive saturates at the start only under the env's own gains: {only}; only under the config's: {ceases}")
    assert only >= 1 and ceases >= 1
    t = r.tables
    assert (t["link_mass_scale"] == 1).all() and (t["restitution_scale"] == 1).all() and (t["friction_scale"] == 1).all()
    assert t["dof_stiffness_scale"].min() < 0.6 and t["dof_stiffness_scale"].max() > 1.4


def shim_steps(oracle_lib, r, what):
    """ShimEnv stepped from each state of run `r` against the oracle: the suite's integers, terms and tolerances (compare_step), the probe's
    set-aside env-steps through check_excluded, and the exactness assertion.  -> exact values checked per tensor."""
    cfg = r.cfg
    s_env = sb.ShimEnv(cfg)
    oa, ra = sc.tolerances(cfg)
    log = ExclusionLog(f"host shim (kernel arithmetic) on the scripted joint limits vs oracle {what}", bound=js.EXCLUDED_CAP)
    o = oracle_lib.OracleEnv(cfg)
    exact = dict(dof_pos=0, dof_vel=0, dof_force=0)
    for t, s in enumerate(r.steps):
        o.set_state(s["st"])
        s_env.copy_state_from(o)
        s_env.step(s["act"])
        log.add(s["keep"])
        r.probe.check_excluded(log, t, s["st"], s["act"], s["main"], s_env, s["keep"], oa, ra)
        sc.compare_step(s_env, s, t, cfg, oa, ra, f"host shim {what}")
        for k, v in js.assert_exact(s_env, s, r.meta, f"host shim {what}, step {t}").items():
            exact[k] += v
    o.close()
    log.close()
    return exact


@pytest.mark.parametrize("variant", js.VARIANTS)
def test_kernel_arithmetic_on_every_drive_cell(oracle_lib, variant):
    """ppenv_device.h compiled for the host (fp32) on the plain run of every variant.  (The host shim has no table-reading step: the
    randomised-gains trajectories are compared on the GPU.)  Exactness, js.exact_masks: where the oracle ends a stop cell's step on the stop
    at rest, ends at the speed cap with its uncapped twin beyond, or reports +-effort with its unlimited twin beyond, the kernel arithmetic's q,
    qd, dof_force of the focus joint are the oracle's fp32 values bit for bit — float32(limit), 0, +-float32(vel_limit), +-float32(effort)."""
    r = js.oracle_run(variant, js.COUNTED, False)
    exact = shim_steps(oracle_lib, r, f"[{variant}, n={js.COUNTED}]")
    print(f"[{variant}] focus-joint values checked bit for bit: {exact}")
    assert min(exact.values()) >= 7 * 2 * js.FLOOR


@pytest.mark.parametrize("n", js.SIZES)
def test_kernel_arithmetic_on_the_ragged_sizes(oracle_lib, n):
    """TT at the sizes the GPU test runs for the ragged workgroups: compared, not counted."""
    r = js.oracle_run("TT", n, False)
    assert r.resets == 0
    shim_steps(oracle_lib, r, f"[TT, n={n}]")
