"""The scripted states of tests/ta_ball_contact_scenarios.py, stepped by the oracle alone: they bring the ball to the blade, the six body shapes and
the bound of a MOVING 27-dof humanoid, and to the scene bodies under the 27-dof constants, often enough for the GPU comparison of
tests/test_ta_ball_contacts_gpu.py to mean something — and the lane path's geometry (collision_geometry in ppenv_ta_device.h, the only copy the
host shim compiles) against the oracle on them.

Neither the free-running rollouts (run_chain_step_parity) nor the reward-branch states (a humanoid standing at rest, the blade edge-on) compare a
contact in which a body's velocity is not zero."""
import numpy as np
import pytest

import shim_binding as sb
import ta_ball_contact_scenarios as sc
import test_ta_physics as tp
from helpers import ExclusionLog
from isaacgym_amd import scene

# what tests/test_ta_ball_contacts_gpu.py runs: the smallest ragged size found (1101 - 1201) at which every cell holds the floor, plain and randomised
SEED, N = 1, 1201


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "randomised_materials"])
def run(request, oracle_lib):
    return (request.param,) + sc.oracle_run(N, SEED, request.param)


def test_every_contact_cell_holds_the_floor(run):
    dr, p, irb, tables, steps = run
    sc.assert_floor(steps, f"oracle [randomised={dr}]")


def test_excluded_share_is_under_the_bound(run):
    dr, p, irb, tables, steps = run
    sc.assert_excluded_share(steps, f"oracle [randomised={dr}]")


def test_no_effect_cells_are_free_flight(run):
    """Inside the bound without a contact, and outside it: the oracle without the whole humanoid gives the same ball, bit for bit."""
    dr, p, irb, tables, steps = run
    for name in sc.NO_EFFECT:
        cell = np.stack([s["cells"][name] for s in steps])
        free = np.stack([s["free"] for s in steps])
        print(f"{name:40s} {int(cell.sum()):5d} env-steps, all free flight: {bool(free[cell].all())}")
        assert cell.sum() >= sc.FLOOR and free[cell].all(), name
    # ... and the bound is not where the standing pose puts it (the root is displaced and rotated): often enough the standing pose's bound would decide
    # the other way about the ball at the step's start
    cfg, m = scene.build_ta_scene(N), scene.build_ta_model()
    stand = sc.Humanoid(cfg, m, irb[:1]).bound
    for name, sign in zip(sc.NO_EFFECT, (1.0, -1.0)):
        other = 0
        for s in steps:
            d = np.linalg.norm(s["root0"][:, 2, 0:3].astype(np.float64) - stand, axis=1) - float(cfg.humanoid_bound_radius)
            other += int((s["cells"][name] & (sign * d > 0)).sum())
        print(f"{name:40s} the standing pose's bound decides the other way in {other} env-steps")
        assert other >= sc.FLOOR, name


def oracle_fk(m, s):
    from oracle import binding
    return binding.ta_forward_kinematics(m, s["root0"], s["dof0"])


def test_moving_cells_depend_on_the_motion(run):
    """Every env-step of a moving cell: the contact point moves at >= MOVING_SPEED and the oracle from the same pose with that link's velocities
    zeroed differs by REACHED x the tolerance; in a substep-1 cell the contact point has travelled >= 20 x TOL["rb_pos"] during substep 0.  The
    at-rest cells are slower than REST_SPEED.  Recomputed here from what oracle_run kept of the oracle's runs."""
    dr, p, irb, tables, steps = run
    travel_min = sc.TRAVEL_FACTOR * tp.TOL["rb_pos"]
    for name in sc.CELLS:
        body = name.split("/")[1] if name.split("/")[0] != "paddle" else "paddle"
        if body not in sc.BODY_LINK:
            continue
        link = sc.BODY_LINK[body]
        cell = np.stack([s["cells"][name] for s in steps])
        speed, travel, sub = (np.stack([s["contact"][body][i] for s in steps])[cell] for i in range(3))
        dep = np.stack([s["veldep"][link] for s in steps])[cell]
        print(f"{name:40s} {int(cell.sum()):4d} env-steps: contact point at {speed.min():.2f} - {speed.max():.2f} m/s, travelled {1e3 * travel.min():.2f} - "
              f"{1e3 * travel.max():.2f} mm in substep 0, {int(dep.sum())} differ from their zero-velocity state by {sc.REACHED:.0f} x the tolerance")
        if name in sc.MOVING_CELLS:
            assert dep.all() and speed.min() >= sc.MOVING_SPEED, name
            assert (sub == (1 if name in sc.SUB1_CELLS else 0)).all(), name
            if name in sc.SUB1_CELLS:
                assert travel.min() >= travel_min, name
        else:
            assert speed.max() < sc.REST_SPEED, name


def test_edge_tolerance_only_where_the_normal_has_a_short_lever(run):
    """The derived tolerance sits on the blade's rim, the capsules' end caps and the table's edge, and nowhere else."""
    dr, p, irb, tables, steps = run
    for s in steps:
        edge_cell = np.any([s["cells"][c] for c in sc.EDGE_CELLS], axis=0)
        other = np.any([s["cells"][c] for c in sc.CELLS if c not in sc.EDGE_CELLS], axis=0)
        assert (s["edge"][edge_cell] > 0).all() and (s["edge"][other & ~edge_cell] == 0).all()
        # 4 x 2^-23 x 3.1 m / 0.02 m x 7 m/s = 5e-4 m/s at the most (3e-4 here): under the suite's own tolerance
        assert s["edge"].max() < tp.TOL["root_vel"]


def test_kernel_arithmetic_on_ball_contacts_with_a_moving_humanoid(oracle_lib):
    """ppenv_ta_device.h compiled for the host (fp32): the lane path's collision_geometry from the scripted states against the oracle at
    check_step's tolerances, and the flags and rewards the oracle's post_physics_step makes of either."""
    p, irb, tables, steps = sc.oracle_run(N, SEED, False)      # (the host shim has no table-reading step: the randomised trajectory is compared on the GPU)
    cfg, m = scene.build_ta_scene(N), scene.build_ta_model()
    from oracle import binding
    log = ExclusionLog("host shim (kernel arithmetic) 27-dof rigid-body step on ball contacts with a moving humanoid vs oracle", bound=sc.EXCLUDED_BOUND)
    for t, s in enumerate(steps):
        r2, d2 = s["root0"].copy(), s["dof0"].copy()
        rb2, frc2, pvx2 = sb.ta_simulate(cfg, m, s["act"], r2, d2)
        root, dof, rb, frc, pvx = s["after_sim"]
        keep = ~(s["switch"] | s["near"])
        np.testing.assert_array_equal(pvx2, pvx)
        log.add(keep)
        tp.ta_sim_check_excluded(log, t, ~keep, (r2, d2, rb2, frc2), (root, dof, rb, frc),
                                 tp.rows_simulate(binding, cfg, m, s["act"], s["root0"], s["dof0"]), seed=6)
        sc.compare_sim((r2, d2, rb2, frc2), (root, dof, rb, frc), keep, s["edge"], cfg, f"scripted contacts, step {t}")
        flags, episode, progress = s["flags0"].copy(), s["episode0"].copy(), s["progress0"].copy()
        _, rew, reset = binding.ta_post_physics_step(p, rb2, irb, r2, d2, frc2, pvx2, None, flags, episode, progress)
        np.testing.assert_array_equal(reset, s["main"][6])
        np.testing.assert_array_equal(flags[keep], s["main"][9][keep])
        tp.assert_close(rew[keep], s["main"][5][keep], f"step {t}: rew", atol=tp.TA_REW_ATOL + abs(float(p.alpha_velocity_reward)) * s["edge"][keep])
    log.close()
