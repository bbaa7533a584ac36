"""The 27-dof step kernels on every regime of joint_torque: the chain-wave kernel (one limb wave per limb, each with its own copy of the limit
and speed-cap arithmetic), the `quad` kernel and the `lane` path, each against the oracle on the scripted states of
tests/ta_joint_limit_scenarios.py — the limit spring's toe and its linear law, its damper moving out and in, the speed-cap damper fading in and
in full, both at once, and the drive saturated before the solve and in the reported dof_force, on every joint and either sign.

Three steps, every step restarted from the oracle's tensors, through test_ta_ball_contacts_gpu.run_kernel: the terms and tolerances of
run_chain_step_parity (test_ta_physics), what is set aside decided by the oracle alone (ball_switch_probe with dof_after +
ta_branch_scenarios.near_threshold), checked by ta_chain_check_excluded and bounded at 2 %; the floor of 8 kept env-steps per
(joint, cell, sign) is asserted over what is left.  TAEnv.set_randomization accepts gain tables, so the table-reading chain kernel runs the same
states with per-env kp / kd scales."""
import pytest

import ta_joint_limit_scenarios as ts
import test_ta_physics as tp
from test_ta_ball_contacts_gpu import run_kernel
from test_ta_joint_limits_host import N, SEED


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,n", [("chain", N), ("quad", N), ("lane", N), ("chain", 50)])
def test_ta_step_kernels_on_every_joint_regime(oracle_lib, monkeypatch, kernel, n):
    """TAEnv.step on each mapping.  n = 50 (one ragged workgroup, the reference's per-env initial_body_states; its 50 envs are the first 50 cases
    of joints 0 - 26) is too small for the floor: it is compared, not counted."""
    from isaacgym_amd.tensor_api import TAEnv
    monkeypatch.setenv("PPENV_TA_KERNEL", kernel)
    r = ts.oracle_run(n, SEED, False, n == 50)
    env = TAEnv(n, device="cuda:0", seed=ts.ENV_SEED, materialize_rb=True, share_initial_rb=(n != 50))
    assert env.sim.kernel == kernel
    label = f"gpu 27-dof {kernel} step on the scripted joint limits vs oracle [n={n}]"
    run_kernel(oracle_lib, env, n, False, n == 50, label, tp._ta_obs_atol(), run=(r.p, r.irb, None, r.steps))
    if n == N:
        ts.assert_floor(r, label)
        ts.assert_excluded_share(r, label)
    env.close()


@pytest.mark.gpu
def test_ta_chain_kernel_with_randomised_gains_on_every_joint_regime(oracle_lib, monkeypatch):
    """The table-reading instantiation of the chain-wave kernel: per-env kp / kd scales in [0.5, 1.5] (they move the saturation point of the
    drive), the oracle through ta_simulate_dr with the same tables, no noise."""
    from isaacgym_amd.tensor_api import TAEnv
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    r = ts.oracle_run(N, SEED, True)
    only, ceases = ts.gain_dependence(r)
    assert only >= 1 and ceases >= 1
    env = TAEnv(N, device="cuda:0", seed=ts.ENV_SEED, materialize_rb=True)
    env.set_randomization(**r.tables, action_noise_sigma=0.0, observation_noise_sigma=0.0)
    label = f"gpu 27-dof chain-wave step with randomised gains on the scripted joint limits vs oracle [n={N}]"
    run_kernel(oracle_lib, env, N, True, False, label, tp._ta_obs_atol(), run=(r.p, r.irb, r.tables, r.steps))
    ts.assert_floor(r, label)
    ts.assert_excluded_share(r, label)
    env.close()
