"""The HIP kernels' per-env arithmetic (isaacgym_amd/csrc/ppenv_device.h, compiled for the host by
tests/csrc/host_shim.cpp) against the CPU oracle.  Runs without a GPU; the same comparisons run on
the real kernels in test_gpu_parity.py."""
import types

import numpy as np
import pytest

import shim_binding as sb
from helpers import RTOL, ExclusionLog, SensitivityProbe, assert_close, assert_state_close, mask_envs, obs_atol, reward_atol
from isaacgym_amd import scene


def test_aba_matches_oracle_forward_dynamics(oracle_lib):
    """fp32 articulated-body algorithm (kernel) vs fp64 Newton-Euler + dense solve (oracle)."""
    cfg = scene.build_config("TT", num_envs=1)
    rng = np.random.default_rng(0)
    for _ in range(300):
        q = rng.uniform(-1.5, 1.5, 7).astype(np.float32)
        qd = rng.uniform(-10, 10, 7).astype(np.float32)
        tau = rng.uniform(-25, 25, 7).astype(np.float32)
        arm = rng.uniform(0, 0.01, 7).astype(np.float32)
        want = oracle_lib.arm_qdd(cfg, q.astype(np.float64), qd.astype(np.float64), tau.astype(np.float64), arm.astype(np.float64))
        got = sb.arm_qdd(cfg, q, qd, tau, arm)
        assert_close(got, want, "qdd", rtol=RTOL, atol=RTOL * np.abs(want).max())


def test_serve_velocity_matches_oracle(oracle_lib):
    for variant in ("T3", "TT", "TN"):
        cfg = scene.build_config(variant, num_envs=1, seed=1234)
        for gid in (0, 1, 77, 16383, 65535):
            for ep in (0, 1, 2, 1000):
                assert_close(sb.serve_velocity(cfg, gid, ep), oracle_lib.serve_velocity(cfg, gid, ep), "serve", atol=2e-6)


@pytest.mark.parametrize("variant", ["TT", "TN", "T3"])
def test_single_step_parity_vs_oracle(oracle_lib, variant):
    """Every step starts both implementations from the oracle's state, so errors do not compound."""
    n = 256
    cfg = scene.build_config(variant, num_envs=n, seed=7)
    o = oracle_lib.OracleEnv(cfg)
    s = sb.ShimEnv(cfg)
    rng = np.random.default_rng(1)
    oa, ra = obs_atol(), reward_atol(cfg)
    resets = 0
    log = ExclusionLog(f"host shim (kernel arithmetic) vs oracle [{variant}]", bound=0.005)
    steps = 180 if variant == "TN" else 120   # TN only ever resets on its 170-step time-out (TN:1317)
    probe = SensitivityProbe(oracle_lib, cfg)
    for t in range(steps):
        actions = rng.uniform(-1.2, 1.2, (n, 7)).astype(np.float32)   # beyond +-1: exercises clipActions
        s.copy_state_from(o)
        st = o.get_state()
        o.step(actions)
        s.step(actions)
        keep = ~probe.sensitive(st, actions, o)   # envs within rounding of a contact switch this step (helpers.SensitivityProbe)
        log.add(keep)
        probe.check_excluded(log, t, st, actions, o, s, keep, oa, ra)
        sm, om = mask_envs(s, keep), mask_envs(o, keep)
        np.testing.assert_array_equal(sm.reset_buf, om.reset_buf, err_msg=f"reset step {t}")
        np.testing.assert_array_equal(sm.progress_buf, om.progress_buf, err_msg=f"progress step {t}")
        np.testing.assert_array_equal(sm.flags, om.flags, err_msg=f"flags step {t}")
        np.testing.assert_array_equal(sm.episode, om.episode, err_msg=f"episode step {t}")
        assert_state_close(sm, om, f"step {t}")
        assert_close(sm.obs_buf, om.obs_buf, f"obs step {t}", atol=oa)
        assert_close(sm.rew_buf, om.rew_buf, f"rew step {t}", atol=ra)
        resets += int(o.reset_buf.sum())
    assert resets > 100
    log.close()


def test_gentle_policy_single_step_is_tight(oracle_lib):
    """With small smooth actions (no flailing at the limits) plain rtol 1e-4 / atol 1e-5 holds.  (The stops, the speed cap and the torque limit
    themselves are not left to flailing: tests/joint_limit_scenarios.py scripts and counts them, tests/test_joint_limits_host.py / _gpu.py.)"""
    n = 128
    cfg = scene.build_config("TT", num_envs=n, seed=3)
    o = oracle_lib.OracleEnv(cfg)
    s = sb.ShimEnv(cfg)
    rng = np.random.default_rng(2)
    a = np.zeros((n, 7), np.float32)
    for t in range(100):
        a = np.clip(a + rng.normal(0, 0.02, (n, 7)), -0.3, 0.3).astype(np.float32)
        s.copy_state_from(o)
        o.step(a)
        s.step(a)
        np.testing.assert_array_equal(s.reset_buf, o.reset_buf)
        assert_close(s.dof_pos, o.dof_pos, "dof_pos", atol=1e-5)
        assert_close(s.dof_vel, o.dof_vel, "dof_vel", atol=1e-4)
        assert_close(s.ball[0:3], o.ball[0:3], "ball pos", atol=1e-5)
        # a ball on the table's edge: the normal is (centre - edge) / 0.02 m, so the 1.2e-7 m quantum of an fp32 x ~ 1.4 m
        # turns into 1e-5 of normal and, at 8 m/s, 2e-4 m/s of rebound velocity
        assert_close(s.ball[7:10], o.ball[7:10], "ball vel", atol=5e-4)
        oa = np.full(80, 1e-4)
        oa[77:80] = 5e-4   # ball velocity columns (TT:1660), as above
        assert_close(s.obs_buf, o.obs_buf, "obs", atol=oa)


def test_free_running_rollout_statistics(oracle_lib):
    """Trajectories diverge chaotically after contacts, so a free-running comparison is statistical."""
    n = 512
    cfg = scene.build_config("TT", num_envs=n, seed=11)
    o = oracle_lib.OracleEnv(cfg)
    s = sb.ShimEnv(cfg)
    s.copy_state_from(o)
    rng = np.random.default_rng(5)
    tot = np.zeros(2)
    resets = np.zeros(2)
    for t in range(300):
        actions = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
        o.step(actions)
        s.step(actions)
        tot += [o.rew_buf.mean(), s.rew_buf.mean()]
        resets += [o.reset_buf.sum(), s.reset_buf.sum()]
    assert abs(resets[0] - resets[1]) <= 0.05 * resets[0] + 5
    assert abs(tot[0] - tot[1]) <= 0.10 * abs(tot[0]) + 5.0


# ------------------------------------------------------------------------------------------- the check of the probe-excluded env-steps
def _copy_view(view):
    return types.SimpleNamespace(**{k: np.array(getattr(view, k)) for k in
                                    ("dof_pos", "dof_vel", "dof_force", "ball", "flags", "episode", "progress_buf", "reset_buf", "rew_buf", "obs_buf")})


def _scratch_log(name):
    """A stand-in ExclusionLog for the corrupted runs: counts only (opening a real one would restart the retained-error record)."""
    return types.SimpleNamespace(name=name, matched_main=0, matched_jittered=0, unmatched=0)


@pytest.mark.parametrize("variant", ["TT", "TN", "T3"])
def test_check_excluded_matches_the_kernel_and_rejects_corrupted_steps(oracle_lib, variant):
    """helpers.check_excluded on the env-steps the probe sets aside: the kernel arithmetic matches the main oracle run or a jittered one
    at every one of them, and the same step with the excluded envs' outputs corrupted (a NaN, ball velocity x 0.97, one flag bit flipped)
    is rejected at every excluded env."""
    n = 256
    cfg = scene.build_config(variant, num_envs=n, seed=7)
    o, s = oracle_lib.OracleEnv(cfg), sb.ShimEnv(cfg)
    rng = np.random.default_rng(1)
    oa, ra = obs_atol(), reward_atol(cfg)
    probe = SensitivityProbe(oracle_lib, cfg)
    log = ExclusionLog(f"check_excluded on the host shim [{variant}]", bound=0.005)

    def nan(v, bad):
        v.dof_vel[2, bad] = np.nan

    def ball_vel(v, bad):
        v.ball[7:10, bad] *= np.float32(0.97)

    def flag_bit(v, bad):
        v.flags[bad] ^= np.uint32(1)
    rejected = dict.fromkeys(("nan", "ball_vel", "flag_bit"), 0)
    for t in range(180 if variant == "TN" else 120):
        actions = rng.uniform(-1.2, 1.2, (n, 7)).astype(np.float32)
        s.copy_state_from(o)
        st = o.get_state()
        o.step(actions)
        s.step(actions)
        keep = ~probe.sensitive(st, actions, o)
        log.add(keep)
        probe.check_excluded(log, t, st, actions, o, s, keep, oa, ra)
        if keep.all():
            continue
        for name, corrupt in (("nan", nan), ("ball_vel", ball_vel), ("flag_bit", flag_bit)):
            v = _copy_view(s)
            corrupt(v, ~keep)
            scratch = _scratch_log(f"{variant} with {name} on the excluded envs")
            with pytest.raises(AssertionError, match="matches neither the main oracle run nor any of 8 jittered runs"):
                probe.check_excluded(scratch, t, st, actions, o, v, keep, oa, ra)
            assert scratch.unmatched == int((~keep).sum()), (name, t, scratch)
            rejected[name] += scratch.unmatched
    log.close()
    assert log.excluded > 5 and all(r == log.excluded for r in rejected.values()), rejected


def test_check_excluded_on_the_27dof_step(oracle_lib):
    """The same for the 27-dof step: the kernel's rigid-body arithmetic (host shim, the second URDF asset: its left sole starts inside the
    ground, test_ta_physics.ball_switch_probe) followed by post_physics_step, checked through test_ta_physics.ta_chain_check_excluded as
    run_chain_step_parity does on the GPU; corrupted outputs of the excluded envs are rejected, also where the envelope of the runs is allowed."""
    import urdf_assets
    from test_ta_physics import _ta_obs_atol, ball_switch_probe, initial_tensors, rows_simulate, ta_chain_check_excluded
    n = 192
    cfg, m = scene.build_ta_scene(n), urdf_assets.second_27dof_model()
    p = scene.build_ta_params(n, env={"episodeLength": 10}, seed=12)
    root, dof = initial_tensors(n, seed=6)
    irb = oracle_lib.ta_forward_kinematics(m, root, dof)
    flags, episode, progress = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int64)
    rng = np.random.default_rng(7)
    oa = _ta_obs_atol()
    log = ExclusionLog("check_excluded on the host shim, 27-dof step of the second asset", bound=0.01)
    rejected = dict.fromkeys(("nan", "ball_vel", "flag_bit"), 0)
    act = None
    for t in range(40):
        if t % 4 == 0:
            act = rng.uniform(-1.2, 1.2, (n, 27)).astype(np.float32)
        root0, dof0 = root.copy(), dof.copy()
        r2, d2 = root.copy(), dof.copy()
        rb2, frc2, pvx2 = sb.ta_simulate(cfg, m, act, r2, d2)
        rb, frc, pvx = oracle_lib.ta_simulate(cfg, m, act, root, dof, threads=8)
        switch = ball_switch_probe(oracle_lib, cfg, m, act, root0, dof0, root, seed=400 + t, dof_after=dof)
        before, after_sim = (flags.copy(), episode.copy(), progress.copy()), (root.copy(), dof.copy(), rb, frc, pvx)
        f2, e2, p2 = (x.copy() for x in before)
        obs2, rew2, reset2 = oracle_lib.ta_post_physics_step(p, rb2, irb, r2, d2, frc2, pvx2, None, f2, e2, p2)
        obs, rew, reset = oracle_lib.ta_post_physics_step(p, rb, irb, root, dof, frc, pvx, None, flags, episode, progress)
        log.add(~switch)
        main = (root, dof, rb, frc, obs, rew, reset, progress, episode, flags)
        simulate = rows_simulate(oracle_lib, cfg, m, act, root0, dof0)
        got = [r2, d2, rb2, frc2, obs2, rew2, reset2, p2, e2, f2]
        ta_chain_check_excluded(oracle_lib, log, t, p, irb, switch, got, main, before, after_sim, simulate, oa, seed=8)
        if switch.any():
            for name in rejected:
                bad = [x.copy() for x in got]
                if name == "nan":
                    bad[1][switch, 5, 1] = np.nan                  # a joint velocity
                elif name == "ball_vel":
                    bad[0][switch, 2, 7:10] *= np.float32(0.97)    # root row 2 = the ball
                else:
                    bad[9][switch] ^= np.uint32(1)
                for envelope in (False, True):        # the envelope of the runs (run_chain_step_parity's joint_probe) rejects them too
                    scratch = _scratch_log(f"27-dof with {name} on the excluded envs")
                    with pytest.raises(AssertionError, match="matches neither the main oracle run nor any of 8 jittered runs"):
                        ta_chain_check_excluded(oracle_lib, scratch, t, p, irb, switch, bad, main, before, after_sim, simulate, oa, seed=8,
                                                envelope=envelope)
                    assert scratch.unmatched == int(switch.sum()), (name, envelope, t, scratch)
                rejected[name] += scratch.unmatched
        flags[switch] = f2[switch]             # continue from a common state
    log.close()
    assert log.excluded > 0 and all(r == log.excluded for r in rejected.values()), rejected
