"""The step kernels' output stores on every alignment class, bit for bit.

The kernels are deterministic, their random numbers are keyed by the global env id, and an env's trajectory does not depend on how many
envs the handle holds.  So a handle of n envs must produce, step after step, exactly the first rows of a larger handle that is stepped on
the same action rows — whatever path the stores of its last workgroup take: 16-byte pieces of a full workgroup, the ragged loop of a
partly filled one, fields of the [field][n] arrays that start at 4, 8 or 12 bytes past a 16-byte boundary.  No tolerance anywhere:
every comparison is torch.equal.

The windows are long enough for every compared env to reset inside them (asserted), so the reset path's stores are covered too."""
import numpy as np
import pytest

from isaacgym_amd import scene

pytestmark = pytest.mark.gpu

STEPS_7DOF = 160
STEPS_TA = 176        # the 27-dof task resets on its time-out alone (TA:1688; episodeLength 160): in a 64-step window no env resets, in this one every env does
TA_COUNT_BITS = 16 | 32 | 64 | 128 | 256      # PP_TA_OUTCOME_*: cleared in ALL envs whenever ANY env resets (TA:1162-1166), so they depend on who else is in the handle


def _actions(rows, cols, steps):
    """[steps, rows, cols] U(-1, 1) from a fixed host generator, on the device."""
    import torch
    rng = np.random.default_rng(0)
    return torch.from_numpy(np.stack([rng.uniform(-1, 1, (rows, cols)).astype(np.float32) for _ in range(steps)])).cuda()


def _first_bad(ok, what):
    """ok: bool [steps, len(what)] on the device -> asserts all, naming the first failing (step, buffer)."""
    ok = ok.cpu().numpy()
    bad = np.argwhere(~ok)
    assert bad.size == 0, f"first mismatch at step {bad[0][0]}: {what[bad[0][1]]}; {len(bad)} mismatching (step, buffer) pairs in all"


def _run_7dof(variant, big_n, small_ns, steps):
    import torch
    from isaacgym_amd.env import PPEnv
    big = PPEnv(scene.build_config(variant, num_envs=big_n, seed=0), device="cuda:0")
    small = [PPEnv(scene.build_config(variant, num_envs=n, seed=0), device="cuda:0") for n in small_ns]
    A = big.num_agents
    act = _actions(big_n * A, scene.NUM_DOF, steps)
    names = ("obs_buf", "rew_buf", "reset_buf", "progress_buf")
    ok = torch.ones(len(small), steps, len(names), dtype=torch.bool, device="cuda")
    seen = torch.zeros(big_n * A, dtype=torch.bool, device="cuda")
    first = None
    for t in range(steps):
        big.step(act[t])
        seen |= big.reset_buf != 0
        if first is None and bool(seen.any()):
            first = t
        for k, e in enumerate(small):
            rows = e.num_rows
            e.step(act[t, :rows].contiguous())
            for j, name in enumerate(names):
                ok[k, t, j] = torch.equal(getattr(e, name), getattr(big, name)[:rows])
    torch.cuda.synchronize()
    for k, e in enumerate(small):
        n = e.num_envs
        _first_bad(ok[k], [f"{variant} n={n} {name}" for name in names])
        # the full state: SoA [field][n] arrays against the first n columns of the big handle's
        for name in ("dof_pos", "dof_vel", "dof_force", "ball"):
            assert torch.equal(getattr(e, name), getattr(big, name)[:, :n]), f"{variant} n={n}: {name} after {steps} steps"
        assert torch.equal(e.flags.reshape(A, n), big.flags.reshape(A, big_n)[:, :n]), f"{variant} n={n}: flags"
        assert torch.equal(e.episode, big.episode[:n]), f"{variant} n={n}: episode"
        assert e.status == 0
    # the reset path is inside the window: every env of every small handle has reset at least once
    rows = max(small_ns) * A
    missing = torch.nonzero(~seen[:rows]).flatten().tolist()
    print(f"{variant}: first reset at step {first}; {int(seen.sum())} of {big_n * A} rows reset within {steps} steps")
    assert not missing, f"{variant}: rows {missing[:8]} never reset within {steps} steps: lengthen the window"
    assert big.status == 0
    for e in small + [big]:
        e.close()


def test_tt_every_alignment_class_bit_for_bit():
    """n = 61, 67, 130: misaligned fields and ragged last workgroups (nvalid 61, 3, 2); 64 and 192: whole 16-byte pieces; 68: aligned fields and a
    ragged last workgroup of one piece (nvalid 4); 1 and 3: one lane, three lanes."""
    _run_7dof("TT", 192, [1, 3, 61, 64, 67, 68, 130], STEPS_7DOF)


def test_t4_every_alignment_class_bit_for_bit():
    """The 4-actor kernel (two arm waves store the dofs, two obs rows per env)."""
    _run_7dof("T4", 128, [1, 63, 64, 65], STEPS_7DOF)


def test_ta_every_alignment_class_bit_for_bit(monkeypatch):
    """The 27-dof chain-wave kernel (64 envs per workgroup): 1, 15, 16, 17 are ragged workgroups (17 x 313 floats is no multiple of 4 either), 64 a
    full one, against the first rows of 128.  Share of the envs that reset inside the window: all of them, once, at the time-out (asserted)."""
    import torch
    from isaacgym_amd.tensor_api import TAEnv
    monkeypatch.setenv("PPENV_TA_KERNEL", "chain")
    big_n, small_ns, steps = 128, [1, 15, 16, 17, 64], STEPS_TA
    big = TAEnv(big_n, device="cuda:0", seed=0)
    small = [TAEnv(n, device="cuda:0", seed=0) for n in small_ns]
    assert all(e.sim.kernel == "chain" for e in small + [big])
    act = _actions(big_n, scene.TA_NUM_DOF, steps)
    names = ("obs_buf", "rew_buf", "reset_buf", "progress_buf")
    ok = torch.ones(len(small), steps, len(names), dtype=torch.bool, device="cuda")
    seen = torch.zeros(big_n, dtype=torch.bool, device="cuda")
    for t in range(steps):
        big.step(act[t])
        seen |= big.reset_buf != 0
        for k, e in enumerate(small):
            e.step(act[t, :e.num_envs].contiguous())
            for j, name in enumerate(names):
                ok[k, t, j] = torch.equal(getattr(e, name), getattr(big, name)[:e.num_envs])
    torch.cuda.synchronize()
    for k, e in enumerate(small):
        n = e.num_envs
        _first_bad(ok[k], [f"TA n={n} {name}" for name in names])
        for name in ("root_states", "dof_states", "dof_force_tensor", "pre_ball_vx"):
            assert torch.equal(getattr(e, name), getattr(big, name)[:n]), f"TA n={n}: {name} after {steps} steps"
        assert torch.equal(e.state.flags & ~TA_COUNT_BITS, big.state.flags[:n] & ~TA_COUNT_BITS), f"TA n={n}: flags"
        assert torch.equal(e.state.episode, big.state.episode[:n]), f"TA n={n}: episode"
        assert e.sim.status == 0
    print(f"TA: {int(seen.sum())} of {big_n} envs reset within {steps} steps")
    assert bool(seen[:max(small_ns)].all()), f"TA: envs {torch.nonzero(~seen[:max(small_ns)]).flatten().tolist()[:8]} never reset within {steps} steps: lengthen the window"
    assert big.sim.status == 0
    for e in small + [big]:
        e.close()


@pytest.mark.parametrize("n", [64, 67])
@pytest.mark.parametrize("rew_off,reset_off", [(1, 1), (2, 3)])     # rew 4 / 8 bytes past a 16-byte boundary; reset (int64) 8 bytes past one
def test_redirected_outputs_do_not_overrun(n, rew_off, reset_off):
    """ppenv_step_into with obs / rew / reset pointing into the middle of larger, canary-filled tensors: after 8 steps the slices hold what a twin
    handle's own buffers hold, and every word outside them is untouched."""
    import torch
    from isaacgym_amd.env import PPEnv
    steps, pad = 8, 64
    env = PPEnv(scene.build_config("TT", num_envs=n, seed=0), device="cuda:0")
    twin = PPEnv(scene.build_config("TT", num_envs=n, seed=0), device="cuda:0")
    act = _actions(n, scene.NUM_DOF, steps)
    F_CANARY, I_CANARY = -12345.5, 0x5A5A5A5A5A5A5A5A
    obs_off = 3 * scene.NUM_OBS                                                 # a multiple of 16 bytes: ppenv_step_into requires it of obs
    obs_big = torch.full((obs_off + n * scene.NUM_OBS + pad,), F_CANARY, device="cuda")
    rew_big = torch.full((rew_off + n + pad,), F_CANARY, device="cuda")
    reset_big = torch.full((reset_off + n + pad,), I_CANARY, dtype=torch.int64, device="cuda")
    assert obs_big.data_ptr() % 16 == 0 and rew_big.data_ptr() % 16 == 0 and reset_big.data_ptr() % 16 == 0
    obs, rew, reset = obs_big[obs_off:obs_off + n * scene.NUM_OBS], rew_big[rew_off:rew_off + n], reset_big[reset_off:reset_off + n]
    assert rew.data_ptr() % 16 == 4 * rew_off and reset.data_ptr() % 16 == 8
    for t in range(steps):
        env.step(act[t], obs=obs, rew=rew, reset=reset)
        twin.step(act[t])
        assert torch.equal(obs.view(n, scene.NUM_OBS), twin.obs_buf), f"obs slice, step {t}"
        assert torch.equal(rew, twin.rew_buf), f"rew slice, step {t}"
        assert torch.equal(reset, twin.reset_buf), f"reset slice, step {t}"
    for name, big, off, length, canary in (("obs", obs_big, obs_off, n * scene.NUM_OBS, F_CANARY), ("rew", rew_big, rew_off, n, F_CANARY),
                                           ("reset", reset_big, reset_off, n, I_CANARY)):
        assert bool((big[:off] == canary).all()) and bool((big[off + length:] == canary).all()), f"{name}: a word outside the slice was written"
    for name in ("dof_pos", "dof_vel", "dof_force", "ball", "progress_buf", "episode", "flags"):
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    assert env.status == 0 and twin.status == 0
    env.close(); twin.close()


def test_graph_replay_equals_eager():
    """32 steps at 130 envs captured into one graph, as bench.py captures a horizon, and replayed: bit for bit the eager 32 steps."""
    import torch
    from isaacgym_amd.env import PPEnv
    n, horizon = 130, 32
    eager = PPEnv(scene.build_config("TT", num_envs=n, seed=0), device="cuda:0")
    graphed = PPEnv(scene.build_config("TT", num_envs=n, seed=0), device="cuda:0")
    pool = list(_actions(n, scene.NUM_DOF, 8))
    with torch.no_grad():
        for s in range(horizon):                 # lazy initialisation must not happen inside the capture
            graphed.step(pool[s & 7])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            for s in range(horizon):
                graphed.step(pool[s & 7])
        g.replay()
        for s in range(2 * horizon):
            eager.step(pool[s & 7])
    torch.cuda.synchronize()
    for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "dof_pos", "dof_vel", "dof_force", "ball", "flags", "episode"):
        assert torch.equal(getattr(graphed, name), getattr(eager, name)), name
    assert graphed.status == 0 and eager.status == 0
    eager.close(); graphed.close()
