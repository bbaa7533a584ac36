"""The 27-dof step kernels on every paying branch of the reward (TA:1440-1690): the chain-wave kernel's hand-written restatement, the
`quad` kernel's ta_task_env<4> on LDS tiles, the `lane` path and the stand-alone post_physics_step kernel, each against the oracle on the
scripted states of tests/ta_branch_scenarios.py.  The free-running rollouts of tests/test_ta_physics.py reach none of these branches.

Two passes of 3 steps, every step restarted from the oracle's tensors: in the first nobody is at the time-out, so the count bits survive
and are compared bit for bit; in the second every 7th env resets in each step — the step its ball was aimed at — so the reward is compared
pre-reset and the observation, the cleared sticky bits and the any-reset clear of the count bits post-reset, on envs that are on a paying
branch in that same step.  Terms and tolerances are those of run_chain_step_parity, imported from test_ta_physics; what is set aside is
decided by the oracle alone (ball_switch_probe + ta_branch_scenarios.near_threshold), must match the oracle's main or a jittered run
(ta_chain_check_excluded), and is bounded at 2 % of the env-steps; the floor of 8 kept env-steps per cell is asserted over what is left."""
import numpy as np
import pytest

import ta_branch_scenarios as sc
import test_ta_physics as tp
from helpers import ExclusionLog, assert_close
from isaacgym_amd import scene

SEED = 1
N = 1000          # the smallest size at which every cell holds the floor in both passes; a ragged last workgroup for chain (64 envs) and quad


def assert_floor(steps, resets, what):
    counts = sc.cell_counts(steps, only_resets=resets)
    low = {k: v for k, v in counts.items() if v < sc.FLOOR}
    assert not low, f"{what}: cells under the floor of {sc.FLOOR} kept env-steps: {low}"


def compare_step(t, got, s, keep, oa):
    """run_chain_step_parity's comparisons of one step: got = the kernel's (root, dof, rb, frc, obs, rew, reset, progress, episode, flags)."""
    g_root, g_dof, g_rb, g_frc, g_obs, g_rew, g_reset, g_progress, g_episode, g_flags = got
    root, dof, rb, frc, obs, rew, reset, progress, episode, flags = s["main"]
    np.testing.assert_array_equal(g_reset, reset)
    np.testing.assert_array_equal(g_progress, progress)
    np.testing.assert_array_equal(g_episode, episode)
    bad = (g_flags != flags) & keep
    assert not bad.any(), (f"step {t}: flags", np.flatnonzero(bad)[:8], [hex(x) for x in g_flags[bad][:8]], [hex(x) for x in flags[bad][:8]])
    assert_close(g_rew[keep], rew[keep], f"step {t}: rew", atol=tp.TA_REW_ATOL)
    # pre-reset physics through the materialised rigid_body_states; post-reset root / dof against the oracle's
    sign = np.sign(np.sum(g_rb[..., 3:7] * rb[..., 3:7], axis=-1, keepdims=True))
    assert_close((g_rb[..., 3:7] * sign)[keep], rb[keep][..., 3:7], f"step {t}: body quat", atol=2e-4)
    tp.check_step((g_root[keep], g_dof[keep], g_rb[keep][:, :40], g_frc[keep]), (root[keep], dof[keep], rb[keep][:, :40], frc[keep]), f"step {t}")
    assert_close(np.delete(g_obs, 120, axis=1)[keep], np.delete(obs, 120, axis=1)[keep], f"step {t}: obs", atol=np.delete(oa, 120))
    bad = (np.abs(g_obs[:, 120].astype(np.float64) - obs[:, 120]) > tp.obs120_tol(oa, obs, obs[:, 120])) & keep
    assert not bad.any(), (f"step {t}: obs column 120", np.flatnonzero(bad)[:5], g_obs[bad, 120][:5], obs[bad, 120][:5])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,n,resets", [("chain", N, False), ("chain", N, True), ("quad", N, False), ("quad", N, True), ("lane", N, False),
                                             ("lane", N, True), ("chain", 50, True)])
def test_ta_step_kernels_on_paying_reward_branches(oracle_lib, monkeypatch, kernel, n, resets):
    """TAEnv.step on each mapping.  n = 50 (one ragged workgroup, the reference's per-env initial_body_states) is too small for the floor:
    it is compared, not counted."""
    import torch
    from isaacgym_amd.tensor_api import TAEnv
    monkeypatch.setenv("PPENV_TA_KERNEL", kernel)
    cfg, m = scene.build_ta_scene(n), scene.build_ta_model()
    p, irb, steps = sc.oracle_run(n, SEED, resets, per_env_irb=(n == 50))
    env = TAEnv(n, device="cuda:0", seed=sc.ENV_SEED, materialize_rb=True, share_initial_rb=(n != 50))
    assert env.sim.kernel == kernel and env.initial_rb_states.shape == irb.shape
    env.initial_rb_states.copy_(torch.from_numpy(irb))
    oa = tp._ta_obs_atol()
    label = f"gpu 27-dof {kernel} step on the paying reward branches vs oracle [n={n}, {'every 7th env resets' if resets else 'no resets'}]"
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
        tp.ta_chain_check_excluded(oracle_lib, log, t, p, irb, aside, got, s["main"], (s["flags0"], s["episode0"], s["progress0"]), s["after_sim"],
                                   tp.rows_simulate(oracle_lib, cfg, m, s["act"], s["root0"], s["dof0"]), oa, seed=5)
        compare_step(t, got, s, ~aside, oa)
        assert int(s["main"][6].sum()) == (len(range(t, n, 7)) if resets else 0)
    log.close()
    assert env.sim.status == 0
    if n == N:
        assert_floor(steps, resets, label)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("resets", [False, True])
def test_ta_post_physics_kernel_on_paying_reward_branches(oracle_lib, resets):
    """The stand-alone ppenv_ta_post_physics_step (ta_task_env<1>) fed the oracle's own post-simulate tensors: the same fp32 inputs, so no env
    is set aside."""
    import torch
    from isaacgym_amd.tensor_api import TAState
    n = N
    p, irb, steps = sc.oracle_run(n, SEED, resets)
    state = TAState(p, device="cuda:0")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    oa = tp._ta_obs_atol()
    keep = np.ones(n, bool)
    for t, s in enumerate(steps):
        state.flags.copy_(torch.from_numpy(s["flags0"].view(np.int32))); state.episode.copy_(torch.from_numpy(s["episode0"].view(np.int32)))
        state.progress_buf.copy_(torch.from_numpy(s["progress0"]))
        root, dof, rb, frc, pvx = s["after_sim"]
        root_d, dof_d = dev(root), dev(dof)
        state.post_physics_step(dev(rb), dev(irb), root_d, dof_d, dev(frc), dev(pvx))
        got = (root_d.cpu().numpy(), dof_d.cpu().numpy(), rb, frc, state.obs_buf.cpu().numpy(), state.rew_buf.cpu().numpy(), state.reset_buf.cpu().numpy(),
               state.progress_buf.cpu().numpy(), state.episode.cpu().numpy().view(np.uint32), state.flags.cpu().numpy().view(np.uint32))
        compare_step(t, got, s, keep, oa)
    assert int(state._any_reset.item()) == 0
    assert_floor(steps, resets, f"stand-alone post_physics_step [{'resets' if resets else 'no resets'}]")
