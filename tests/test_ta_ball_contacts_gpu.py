"""The 27-dof step kernels on ball contacts with a MOVING humanoid: the chain-wave kernel (limb waves hand the geometry to the ball wave through
LDS slots, one per substep), the `quad` kernel (geometry gathered per limb lane through masks and shuffles) and the `lane` path, each against the
oracle on the scripted states of tests/ta_ball_contact_scenarios.py — the blade's faces, rim and inside, the six body shapes, the bound riding on a
displaced, rotated root, and the scene bodies under the 27-dof constants; at rest and moving, in substep 0 and in substep 1.

Three steps, every step restarted from the oracle's tensors.  Terms and tolerances are those of run_chain_step_parity, imported from
test_ta_physics; the blade's rim, the capsules' end caps and the table's edge carry the derived edge tolerance on the ball's
velocity, its spin, the observation's ball-velocity columns and alpha |vx|, and on nothing else.  What is set aside is decided by the oracle alone
(ball_switch_probe with dof_after + ta_branch_scenarios.near_threshold), must match the oracle's main or a jittered run (ta_chain_check_excluded),
and is bounded at 2 % of the env-steps; the floor of 8 kept env-steps per cell is asserted over what is left."""
import numpy as np
import pytest

import ta_ball_contact_scenarios as sc
import test_ta_physics as tp
from helpers import ExclusionLog
from isaacgym_amd import scene
from test_ta_ball_contacts_host import N, SEED


def run_kernel(oracle_lib, env, n, dr, per_env_irb, label, oa, run=None):
    """run: (params, irb, tables, steps) of another scripted suite's oracle_run with this module's step dicts (tests/test_ta_joint_limits_gpu.py)."""
    import torch
    cfg, m = scene.build_ta_scene(n), scene.build_ta_model()
    p, irb, tables, steps = sc.oracle_run(n, SEED, dr, per_env_irb) if run is None else run
    assert env.initial_rb_states.shape == irb.shape
    env.initial_rb_states.copy_(torch.from_numpy(irb))
    log = ExclusionLog(label, bound=sc.EXCLUDED_BOUND)
    for t, s in enumerate(steps):
        tp.load_chain_state(env, s["root0"], s["dof0"], s["flags0"], s["episode0"], s["progress0"])
        env.step(torch.from_numpy(s["act"]).cuda())
        np.testing.assert_array_equal(env.pre_ball_vx.cpu().numpy(), s["after_sim"][4])
        got = (env.root_states.cpu().numpy(), env.dof_states.cpu().numpy(), env._rb_states.cpu().numpy(), env.dof_force_tensor.cpu().numpy(),
               env.obs_buf.cpu().numpy(), env.rew_buf.cpu().numpy(), env.reset_buf.cpu().numpy(), env.progress_buf.cpu().numpy(),
               env.state.episode.cpu().numpy().view(np.uint32), env.state.flags.cpu().numpy().view(np.uint32))
        aside = s["switch"] | s["near"]
        log.add(~aside)
        simulate = tp.rows_simulate(oracle_lib, cfg, m, s["act"], s["root0"], s["dof0"])
        if dr:                                                # the tables are per env id: every row is stepped, the excluded ones kept
            sim = sc.simulator(oracle_lib, cfg, m, tables, p.seed, p.env_id_offset, s["episode0"], s["progress0"])

            def simulate(envs, scale, rng, s=s, sim=sim):
                rj, dj = tp.jittered(s["root0"], scale, rng), tp.jittered(s["dof0"], scale, rng)
                return tuple(x[envs] for x in (rj, dj) + sim(s["act"], rj, dj))
        tp.ta_chain_check_excluded(oracle_lib, log, t, p, irb, aside, got, s["main"], (s["flags0"], s["episode0"], s["progress0"]), s["after_sim"],
                                   simulate, oa, seed=5)
        sc.compare_step(t, got, s, ~aside, oa, cfg, p.alpha_velocity_reward)
        assert int(s["main"][6].sum()) == 0                   # nobody times out: the trajectory stays the aimed one
    log.close()
    assert env.sim.status == 0
    return steps


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,n", [("chain", N), ("quad", N), ("lane", N), ("chain", 50)])
def test_ta_step_kernels_on_ball_contacts_with_a_moving_humanoid(oracle_lib, monkeypatch, kernel, n):
    """TAEnv.step on each mapping.  n = 50 (one ragged workgroup, the reference's per-env initial_body_states) is too small for the floor: it is
    compared, not counted."""
    from isaacgym_amd.tensor_api import TAEnv
    monkeypatch.setenv("PPENV_TA_KERNEL", kernel)
    env = TAEnv(n, device="cuda:0", seed=sc.ENV_SEED, materialize_rb=True, share_initial_rb=(n != 50))
    assert env.sim.kernel == kernel
    label = f"gpu 27-dof {kernel} step on ball contacts with a moving humanoid vs oracle [n={n}]"
    steps = run_kernel(oracle_lib, env, n, False, n == 50, label, tp._ta_obs_atol())
    if n == N:
        sc.assert_floor(steps, label)
        sc.assert_excluded_share(steps, label)
    env.close()


@pytest.mark.gpu
def test_ta_chain_kernel_with_randomised_materials_on_ball_contacts(oracle_lib, monkeypatch):
    """The table-reading instantiation of the chain-wave kernel: per-env restitution and friction scales (gains and masses stay at 1, so the aimed
    states still land), the oracle through ta_simulate_dr with the same tables.  In the paddle and shape groups the scaled restitution is clamped
    at restitution_max, elsewhere it is not."""
    from isaacgym_amd.tensor_api import TAEnv
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    cfg = scene.build_ta_scene(N)
    tables = sc.dr_tables(N, SEED)
    es, clamp = tables["restitution_scale"], sc.groups_of(N)[0] <= 6
    shapes = [cfg.shape[k].restitution for k in range(cfg.num_shapes)]
    assert cfg.paddle_restitution * es[clamp].min() > cfg.restitution_max and min(shapes) * es[clamp].min() > cfg.restitution_max
    assert max([cfg.paddle_restitution, cfg.ground_restitution, cfg.table.restitution, cfg.net.restitution] + shapes) * es[~clamp].max() < cfg.restitution_max
    env = TAEnv(N, device="cuda:0", seed=sc.ENV_SEED, materialize_rb=True)
    env.set_randomization(**tables, action_noise_sigma=0.0, observation_noise_sigma=0.0)
    label = f"gpu 27-dof chain-wave step with randomised materials on ball contacts with a moving humanoid vs oracle [n={N}]"
    steps = run_kernel(oracle_lib, env, N, True, False, label, tp._ta_obs_atol())
    sc.assert_floor(steps, label)
    sc.assert_excluded_share(steps, label)
    env.close()
