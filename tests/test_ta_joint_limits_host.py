"""The scripted states of tests/ta_joint_limit_scenarios.py, stepped by the oracle alone: every joint of the 27-dof tree in the limit spring's toe and
beyond it, moving out and in, over its speed cap in the fade-in and the full regime, both at once, and with its drive saturated before the solve and
in the reported dof_force — at least FLOOR kept env-steps per (joint, cell, sign), at most 2 % of the env-steps set aside, nobody resetting; then
joint_torque as the lane path compiles it for the host (sb.ta_simulate) against the oracle on them, and the flags and rewards the oracle's
post_physics_step makes of either.  The HIP kernels run the same states in tests/test_ta_joint_limits_gpu.py."""
import numpy as np
import pytest

import shim_binding as sb
import ta_ball_contact_scenarios as bc
import ta_joint_limit_scenarios as ts
import test_ta_physics as tp
from helpers import ExclusionLog

SEED, N = 1, ts.COUNTED        # what tests/test_ta_joint_limits_gpu.py counts


@pytest.fixture(scope="module")
def run(oracle_lib):
    return ts.oracle_run(N, SEED)


def test_counted_size_is_ragged_and_whole_cycles():
    assert N % 64 and N % (27 * len(ts.CASES)) == 0 and sorted(set(c for c, _ in ts.CASES)) == sorted(ts.CELL_NAMES)


def test_every_cell_holds_the_floor(run):
    ts.assert_floor(run, f"oracle [n={N}]")


def test_excluded_share_is_under_the_bound_and_nobody_resets(run):
    ts.assert_excluded_share(run, f"oracle [n={N}]")
    assert all(np.isfinite(x).all() for s in run.steps for x in s["after_sim"])


def test_randomised_gains_run_holds_the_floor_and_moves_the_saturation_point(oracle_lib):
    """The oracle trajectory of the GPU's table-reading case (per-env kp / kd scales on every oracle involved): the floor, the bound, and from the
    tables: env-steps whose focus drive saturates at the step's start only under the env's own gains, and env-steps in which it ceases to."""
    r = ts.oracle_run(N, SEED, True)
    ts.assert_floor(r, f"oracle [n={N}, randomised gains]")
    ts.assert_excluded_share(r, f"oracle [n={N}, randomised gains]")
    only, ceases = ts.gain_dependence(r)
    print(f"env-steps whose focus drive saturates only under the env's own gains: {only}; only under the model's: {ceases}")
    assert only >= 1 and ceases >= 1


def test_every_cell_is_what_it_says(run):
    """Recomputed from the oracle's tensors at the start of every step and the model: where a cell's env-steps stand against the limits and the
    speed cap, and that the torque cells end at +-effort or start beyond it."""
    J, joint, env = ts.joint_table(run.m), run.meta["joint"], np.arange(N)
    h = float(run.cfg.dt) / run.cfg.substeps
    for s in run.steps:
        q0, v0 = s["dof0"][env, joint, 0].astype(np.float64), s["dof0"][env, joint, 1].astype(np.float64)
        frc = s["after_sim"][3][env, joint]
        for sign, name in ((1.0, "upper"), (-1.0, "lower")):
            L = np.array([getattr(run.m.link[j + 1], name) for j in joint], np.float32).astype(np.float64)
            out, ex = (q0 - L) * sign, v0 * sign - J["vel_limit"][joint]
            c = lambda cell: s["cells"][f"{cell}/{name}"]
            for cell in ("limit/toe", "limit/toe_moving_out", "limit/toe_moving_in"):
                assert ((out[c(cell)] > 0) & (out[c(cell)] < 0.01)).all(), cell
            assert (v0[c("limit/toe_moving_out")] * sign >= 1).all() and (v0[c("limit/toe_moving_in")] * sign <= -1).all()
            assert (out[c("limit/linear")] >= 0.01).all()
            assert ((ex[c("speed_cap/fade_in")] > 0) & (ex[c("speed_cap/fade_in")] < 1) & (out[c("speed_cap/fade_in")] <= 0)).all()
            assert ((ex[c("speed_cap/full")] >= 1) & (out[c("speed_cap/full")] <= 0)).all()
            assert ((ex[c("both")] > 0) & (out[c("both")] > 0)).all()
            eff = np.array([run.m.link[j + 1].effort for j in joint], np.float32)
            assert (frc[c("torque/reported")] == np.float32(sign) * eff[c("torque/reported")]).all()
            target = 0.5 * (J["upper"] + J["lower"])[joint] + 0.5 * (J["upper"] - J["lower"])[joint] * np.clip(s["act"][env, joint].astype(np.float64), -1, 1)
            tau0 = J["kp"][joint] * (target - q0 - h * v0) - J["kd"][joint] * v0
            assert (tau0[c("torque/solve")] * sign > eff[c("torque/solve")]).all()


def test_kernel_arithmetic_on_every_joint_regime(run, oracle_lib):
    """ppenv_ta_device.h compiled for the host (fp32): joint_torque on the scripted states against the oracle at check_step's tolerances, the
    set-aside env-steps through ta_sim_check_excluded, and the flags and rewards the oracle's post_physics_step makes of either.  (The host shim
    has no table-reading step, and TAEnv.set_randomization's gain tables are compared on the GPU.)"""
    cfg, m, p, irb = run.cfg, run.m, run.p, run.irb
    log = ExclusionLog("host shim (kernel arithmetic) 27-dof rigid-body step on the scripted joint limits vs oracle", bound=ts.EXCLUDED_BOUND)
    for t, s in enumerate(run.steps):
        r2, d2 = s["root0"].copy(), s["dof0"].copy()
        rb2, frc2, pvx2 = sb.ta_simulate(cfg, m, s["act"], r2, d2)
        root, dof, rb, frc, pvx = s["after_sim"]
        keep = ~(s["switch"] | s["near"])
        np.testing.assert_array_equal(pvx2, pvx)
        log.add(keep)
        tp.ta_sim_check_excluded(log, t, ~keep, (r2, d2, rb2, frc2), (root, dof, rb, frc), tp.rows_simulate(oracle_lib, cfg, m, s["act"], s["root0"], s["dof0"]), seed=6)
        bc.compare_sim((r2, d2, rb2, frc2), (root, dof, rb, frc), keep, s["edge"], cfg, f"scripted joint limits, step {t}")
        flags, episode, progress = s["flags0"].copy(), s["episode0"].copy(), s["progress0"].copy()
        _, rew, reset = oracle_lib.ta_post_physics_step(p, rb2, irb, r2, d2, frc2, pvx2, None, flags, episode, progress)
        np.testing.assert_array_equal(reset, s["main"][6])
        np.testing.assert_array_equal(flags[keep], s["main"][9][keep])
        tp.assert_close(rew[keep], s["main"][5][keep], f"step {t}: rew", atol=tp.TA_REW_ATOL)
    log.close()
