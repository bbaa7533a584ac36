"""The scripted states of tests/ta_branch_scenarios.py, stepped by the oracle alone: they reach every paying branch of the 27-dof reward
(TA:1440-1690) often enough for the GPU comparison of tests/test_ta_reward_branches_gpu.py to mean something.

The free-running parity rollouts (run_chain_step_parity: 640 envs, 90 steps) reach none of these cells: there the oracle sets
HUMANOID_DIE_CALC and FALL_DOWN and nothing else.  Here it sets every count bit and every sticky bit."""
import numpy as np
import pytest

import shim_binding as sb
import ta_branch_scenarios as sc
import test_ta_physics as tp
from helpers import ExclusionLog
from isaacgym_amd import scene

SEED, N = 1, 1000          # what tests/test_ta_reward_branches_gpu.py runs


@pytest.fixture(scope="module", params=[False, True], ids=["no_resets", "every_7th_env_resets"])
def run(request, oracle_lib):
    return (request.param,) + sc.oracle_run(N, SEED, request.param)


def test_every_branch_cell_holds_the_floor(run):
    """At least FLOOR env-steps in every cell after the exclusions; in the reset pass only the env-steps that reset count, so every cell
    coincides with the in-kernel reset that often."""
    resets, p, irb, steps = run
    counts, before = sc.cell_counts(steps, only_resets=resets), sc.cell_counts(steps, keep=[np.ones(N, bool)] * sc.STEPS, only_resets=resets)
    for name in sc.CELLS:
        print(f"{name:42s} {counts[name]:5d} kept of {before[name]}")
    low = {k: v for k, v in counts.items() if v < sc.FLOOR}
    assert not low, f"cells under the floor of {sc.FLOOR} kept env-steps: {low}"


def test_excluded_share_is_under_the_bound(run):
    resets, p, irb, steps = run
    aside = sum(int((s["switch"] | s["near"]).sum()) for s in steps)
    near, switch = sum(int(s["near"].sum()) for s in steps), sum(int(s["switch"].sum()) for s in steps)
    print(f"set aside {aside} of {N * sc.STEPS} env-steps ({100 * aside / (N * sc.STEPS):.3f} %): {near} near a threshold, {switch} on a contact switch")
    assert aside <= sc.EXCLUDED_BOUND * N * sc.STEPS


def test_oracle_sets_every_count_bit_and_every_sticky_bit(run):
    """The gap in the positive: what the rollouts never see.  Without resets every count bit and every sticky bit is newly set somewhere; with
    them, an env that resets has its sticky bits cleared and the count bits are cleared in every env (TA:1021-1024, 1162-1166) — after having
    paid: the reward of those env-steps holds the branch's term."""
    resets, p, irb, steps = run
    new = np.bitwise_or.reduce([s["main"][9] & ~s["flags0"] for s in steps], axis=None)
    timeouts = [int(s["main"][6].sum()) for s in steps]
    if not resets:
        assert timeouts == [0] * sc.STEPS
        for name, bit in {**sc.COUNT_BITS, **sc.STICKY_BITS}.items():
            assert new & bit, f"the oracle never sets {name}"
    else:
        assert timeouts == [len(range(t, N, 7)) for t in range(sc.STEPS)]
        for s in steps:
            rst = s["main"][6] != 0
            assert not (s["main"][9] & scene.TA_COUNT_MASK).any() and not (s["main"][9][rst] & 0xF).any()
            assert (s["main"][7][rst] == 0).all() and (s["main"][8][rst] == s["episode0"][rst] + 1).all()
            paid = s["cells"]["hit_paddle/paid"] & rst
            if paid.any():                                    # alpha |vx| with vx > 1.5: the reward was computed before the reset
                assert (s["main"][5][paid] > 0.9 * p.alpha_velocity_reward * 1.5).all()
            paid = s["cells"]["below/paid"] & rst & ~s["cells"]["x_close/paddle_cond_set"]
            assert (s["main"][5][paid] < 0.5 * p.die_penalty).all()


def test_launch_lands_where_it_aims(oracle_lib):
    """`launch` is the oracle's free flight backwards: a ball started there is at the target after k steps."""
    n = 64
    cfg, m = scene.build_ta_scene(n), scene.build_ta_model()
    rng = np.random.default_rng(0)
    target = np.stack([rng.uniform(1.8, 3.0, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.9, 1.3, n)], axis=1)
    vel = np.stack([rng.uniform(1, 6, n), rng.uniform(-1, 1, n), rng.uniform(-2, 2, n)], axis=1)
    k = np.arange(n) % 4
    root, dof = tp.initial_tensors(n)
    root[:, 2, 0:3], root[:, 2, 7:10] = sc.launch(cfg, target, vel, k), vel
    act = np.zeros((n, 27), np.float32)
    for t in range(4):
        at = k == t
        np.testing.assert_allclose(root[at, 2, 0:3], target[at], atol=2e-6)
        oracle_lib.ta_simulate(cfg, m, act, root, dof, threads=4)


def test_kernel_arithmetic_on_paying_reward_branches(run):
    """ppenv_ta_device.h compiled for the host (fp32) from the scripted states — bounces off the blade's rim, a humanoid dropped into the
    ground — against the oracle at check_step's tolerances, and the flags and rewards the oracle's post_physics_step makes of either."""
    resets, p, irb, steps = run
    cfg, m = scene.build_ta_scene(N), scene.build_ta_model()
    from oracle import binding
    log = ExclusionLog(f"host shim (kernel arithmetic) 27-dof rigid-body step on the scripted states vs oracle [resets={resets}]", bound=sc.EXCLUDED_BOUND)
    for t, s in enumerate(steps):
        r2, d2 = s["root0"].copy(), s["dof0"].copy()
        rb2, frc2, pvx2 = sb.ta_simulate(cfg, m, s["act"], r2, d2)
        root, dof, rb, frc, pvx = s["after_sim"]
        keep = ~(s["switch"] | s["near"])
        np.testing.assert_array_equal(pvx2, pvx)
        log.add(keep)
        tp.ta_sim_check_excluded(log, t, ~keep, (r2, d2, rb2, frc2), (root, dof, rb, frc), tp.rows_simulate(binding, cfg, m, s["act"], s["root0"], s["dof0"]), seed=6)
        tp.check_step((r2[keep], d2[keep], rb2[keep], frc2[keep]), (root[keep], dof[keep], rb[keep], frc[keep]), f"scripted states, step {t}")
        flags, episode, progress = s["flags0"].copy(), s["episode0"].copy(), s["progress0"].copy()
        _, rew, reset = binding.ta_post_physics_step(p, rb2, irb, r2, d2, frc2, pvx2, None, flags, episode, progress)
        np.testing.assert_array_equal(reset, s["main"][6])
        np.testing.assert_array_equal(flags[keep], s["main"][9][keep])
        tp.assert_close(rew[keep], s["main"][5][keep], f"step {t}: rew", atol=tp.TA_REW_ATOL)
    log.close()
