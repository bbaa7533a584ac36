"""The surface every task's env has (isaacgym_amd.dr.NativeEnv), on live tasks of the five registry names, 8 envs each: the attributes
are there and mean what the contract says — the tensors are the ones the step writes, the tables' rows, limits and dt are the task's own —
and the two things the 27-dof task no longer restates (VecTask.step with its own two means, VecTask.reset_idx over TAEnv.reset_all)
compute what they did.  Need a real MI355X."""
import ctypes as C

import numpy as np
import pytest

from isaacgym_amd import scene

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
NAMES = ["HumanoidPingpongG1", TT, "HumanoidPingpongTiltNoEarlyStopG1", T4, TA]
N = 8
ROWS_7DOF = {"dof_stiffness_scale": 7, "dof_damping_scale": 7, "link_mass_scale": 7, "restitution_scale": 0, "friction_scale": 0}
ROWS_27DOF = {"dof_stiffness_scale": 27, "dof_damping_scale": 27, "link_mass_scale": 28, "restitution_scale": 0, "friction_scale": 0}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def make(name, seed=3, **top):
    import isaacgym_amd
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[name])
    env_keys = {k: top.pop(k) for k in list(top) if k == "controlFrequencyInv"}
    cfg["env"].update(env_keys)
    cfg.update(top)
    return isaacgym_amd.make(seed=seed, task=name, num_envs=N, cfg=cfg)


def fixed_actions(torch, task):
    return torch.full((task.num_envs * task.num_agents, task.num_actions), 0.25, device="cuda:0")


@pytest.mark.parametrize("name", NAMES)
def test_surface_of_a_live_task(torch_cuda, name):
    torch = torch_cuda
    task = make(name)
    env, ta = task.env, name == TA
    A = 2 if name == T4 else 1
    assert (env.num_envs, env.num_agents, task.num_agents) == (N, A, A) and env.num_rows == env.num_envs * env.num_agents
    assert env.device == torch.device("cuda:0") and env.L is not None and (not ta or env.L is env.sim.L)
    for t, dtype in ((env.obs_buf, torch.float32), (env.rew_buf, torch.float32), (env.reset_buf, torch.int64), (env.progress_buf, torch.int64)):
        assert t.shape[0] == env.num_rows and t.dtype == dtype
    # episode / flags: the storage the step writes, not a copy
    if ta:
        assert env.episode is env.state.episode and env.flags is env.state.flags
        written = env.state.episode.data_ptr(), env.state.flags.data_ptr()
    else:
        b = scene.Buffers()
        assert env.L.ppenv_buffers_of(env.h, C.byref(b)) == 0
        written = b.episode, b.flags
    assert (env.episode.data_ptr(), env.flags.data_ptr()) == written
    assert env.episode.dtype == env.flags.dtype == torch.int32 and env.episode.shape == (N,) and env.flags.numel() == A * N
    assert env.DR_TABLE_ROWS == (ROWS_27DOF if ta else ROWS_7DOF) and env.dr_tables is None
    # joint limits and names: the scene functions on the task's own config / model
    D = env.num_dofs
    assert D == (27 if ta else 7 * A)
    want, want_names = scene.ta_joint_limits(env.sim.model) if ta else scene.joint_limits(task.native_config, A)
    got, names = env.joint_limits()
    assert got.dtype == np.float32 and got.shape == (D, 4) and np.array_equal(got, want) and names == want_names and len(names) == D
    # joint views: [N, D] float32 views of the env's own tensors
    views = env.joint_views()
    assert len(views) == 3 and all(v.dtype == torch.float32 and tuple(v.shape) == (N, D) for v in views)
    if ta:
        ptrs = (env.dof_states.data_ptr(), env.dof_states.data_ptr() + 4, env.dof_force_tensor.data_ptr())
    else:
        ptrs = (env.dof_pos.data_ptr(), env.dof_vel.data_ptr(), env.dof_force.data_ptr())
    assert tuple(v.data_ptr() for v in views) == ptrs
    assert env.control_dt == (float(env.sim.scene.dt) if ta else float(task.native_config.dt)) and isinstance(env.control_dt, float)
    a = fixed_actions(torch, task)
    task.step(a)
    task.step(a)
    torch.cuda.synchronize()
    assert env.status == 0
    g = env.base_gravity_z
    assert g == (scene.TA_GRAVITY_Z if ta else float(task.native_config.gravity_z)) and g < 0.0
    env.set_gravity(-5.0)
    assert env.base_gravity_z == g
    q, qd, tau = (v.clone() for v in views)                     # the views read what the two steps wrote
    if ta:
        assert torch.equal(q, env.dof_states[:, :, 0]) and torch.equal(qd, env.dof_states[:, :, 1]) and torch.equal(tau, env.dof_force_tensor)
    else:
        assert torch.equal(q, env.dof_pos.T) and torch.equal(qd, env.dof_vel.T) and torch.equal(tau, env.dof_force.T)


def test_control_dt_follows_control_frequency_inv(torch_cuda):
    one, two = make(TT), make(TT, controlFrequencyInv=2)
    assert two.env.control_dt == 2.0 * one.env.control_dt == float(two.native_config.dt)


@pytest.mark.parametrize("name", [TT, TA])
def test_exported_means(torch_cuda, name):
    """stats_every = 1: the one step exports the two means — the 27-dof task's two torch reductions, the 7-dof tasks' reduction launch."""
    torch = torch_cuda
    task = make(name, stats_every=1)
    _, _, _, extras = task.step(fixed_actions(torch, task))
    if name == TA:
        assert torch.equal(extras["reward_mean"], task.rew_buf.mean())
        assert torch.equal(extras["progress_mean"], task.progress_buf.float().mean())
    else:
        s = task.env.reduce_stats(out=torch.zeros(4, dtype=torch.float64, device="cuda:0"))
        assert torch.equal(extras["reward_mean"], (s[0] / s[3]).float())
        assert torch.equal(extras["progress_mean"], (s[1] / s[3]).float())
    assert extras["reward_mean"].dim() == 0 and extras["reward_mean"].device.type == "cuda"


def test_27dof_reset_idx_is_the_envs_reset(torch_cuda):
    """VecTask.reset_idx() on the 27-dof task (-> TAEnv.reset_all) against env.reset_idx(None) on a twin of the same seed, after the same
    three steps: byte-equal state."""
    torch = torch_cuda
    task, twin = make(TA, seed=5), make(TA, seed=5)
    a = fixed_actions(torch, task)
    for _ in range(3):
        task.step(a)
        twin.step(a)
    task.reset_idx()
    twin.env.reset_idx(None)
    raw = lambda t: t.cpu().numpy().tobytes()
    for get in (lambda t: t.env.root_states, lambda t: t.env.dof_states, lambda t: t.env.state.episode, lambda t: t.progress_buf,
                lambda t: t.env.state.flags):
        assert raw(get(task)) == raw(get(twin))
    assert int(task.env.state.episode.min()) >= 1 and not bool(task.progress_buf.any())       # the reset did happen
