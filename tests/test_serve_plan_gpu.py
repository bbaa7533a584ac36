"""The serve plan on the MI355X (include/ppenv_serve.h; PPEnv / TAEnv / VecTask .set_serve_plan).

The kernels against their host build (tests/csrc/serve_shim.cpp, itself pinned to a numpy restatement by tests/test_serve_plan_host.py), bit
for bit: both are compiled unfused.  Then the part no host build can show: that the step kernels CONSUME the buffer — an env that resets in
a step is served exactly the row the buffer held before that step — on the 7-dof, the 4-actor and the 27-dof task; that paired groups
with equal cells are bitwise replicas; that clearing the plan gives the built-in serves back; and that a captured step + apply pair
replays like eager launches.  The tasks run with a short env.episodeLength so that every env resets several times.  Need a real MI355X."""
import numpy as np
import pytest

import serve_shim_binding as ssb
from isaacgym_amd import _lib, scene, serve
from test_play_gpu import make_plain, torch_cuda        # noqa: F401  (a helper and a fixture)

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
SOA, AOS = _lib.SERVE_LAYOUT_SOA3, _lib.SERVE_LAYOUT_AOS5
L_EP = 10                                                        # env.episodeLength of the tasks below


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def host_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ 6. kernel = shim, bitwise
def device_plan(torch, n, cells, form, layout, reset_rows, seed, env_id_offset, paired):
    out = torch.zeros((3, n) if layout == SOA else (n, 5), dtype=torch.float32, device=DEV)
    return serve.ServePlan(_lib.lib(), DEV, n, cells, ssb.DEFAULTS, serve.AXES_27DOF, out, form, layout, reset_rows, seed, env_id_offset, paired)


@pytest.mark.parametrize("S,G", [(1, 1), (63, 1), (64, 1), (65, 1), (257, 1), (300, 1), (65, 2), (100, 3), (1, 5)])
def test_kernel_is_the_host_build(torch_cuda, S, G):
    torch = torch_cuda
    n, steps = S * G, 30
    cells = [{"serve_speed": (6.0 + g, 6.5 + g), "serve_tilt": (-7.0, 3.0 + g), "ball_y": (-0.3, 0.1 * g)} for g in range(G)]
    seed, off = scene.stream_seed(11, scene.STREAM_SERVES), 1000
    for case, (layout, reset_rows, paired) in enumerate((l, r, p) for l in (SOA, AOS) for r in (1, 2) for p in (False, True)):
        form = (scene.VARIANT_TT, scene.VARIANT_TN, scene.VARIANT_T3, scene.VARIANT_T4)[case % 4]
        host = ssb.HostServe(n, cells, form, layout, reset_rows=reset_rows, seed=seed, env_id_offset=off, paired=paired)
        dev = device_plan(torch, n, cells, form, layout, reset_rows, seed, off, paired)
        what = (S, G, layout, reset_rows, paired)
        assert np.array_equal(bits(dev.out), host_bits(host.out)) and int(dev.count.sum()) == 0, what        # the fill
        script = ssb.scripted_resets(steps, n, reset_rows, seed=7 + case)
        for t in range(steps):
            before_out, before_count = dev.out.clone(), dev.count.clone()
            if t == steps // 2:                                                  # one id call in the middle, with ids outside [0, n) and a duplicate
                ids = np.array([0, n - 1, n // 2, -1, n, n + 7, 2 ** 40, 0], np.int64)
                host.apply_ids(ids)
                dev.apply_ids(torch.from_numpy(ids))
                fired = np.zeros(n, bool)
                fired[[0, n - 1, n // 2]] = True
            else:
                host.apply(script[t])
                dev.apply(torch.from_numpy(script[t]).to(DEV))
                fired = script[t][::reset_rows] != 0
            assert np.array_equal(bits(dev.out), host_bits(host.out)), (what, t)
            assert np.array_equal(dev.count.cpu().numpy().view(np.uint32), host.count), (what, t)
            keep = torch.from_numpy(~fired).to(DEV)
            same = (dev.out[:, keep] if layout == SOA else dev.out[keep]), (before_out[:, keep] if layout == SOA else before_out[keep])
            assert np.array_equal(bits(same[0]), bits(same[1])) and torch.equal(dev.count[keep], before_count[keep]), (what, t)
        assert int(host.count.max()) >= 4 or n == 1


# ------------------------------------------------------------------------------------------------------ 7. the step consumes the buffer
def group_cells(name):
    """two cells with disjoint speed ranges; everything else the task's configured range"""
    return [{"serve_speed": (4.0, 4.4)}, {"serve_speed": (6.0, 6.4)}] if name == TA else [{"serve_speed": (6.0, 6.5)}, {"serve_speed": (9.0, 9.5)}]


def ball_rows(task, name):
    """[N, 5] y, z, v_x, v_y, v_z of the ball now (y, z read for the 27-dof task only)"""
    if name == TA:
        r = task.root_states[:, 2]
    else:
        r = task.env.refresh_root_states()[:, task.num_agents + 1]
    return r[:, [1, 2, 7, 8, 9]]


@pytest.mark.parametrize("name", [TT, T4, TA])
def test_step_consumes_the_buffer(torch_cuda, name):
    torch = torch_cuda
    n, S = 130, 65
    task = make_plain(name, n, 5, episode_length=L_EP)
    cells = group_cells(name)
    plan = task.set_serve_plan(cells)
    assert plan is task.env.serve_plan and tuple(plan.out.shape) == ((n, 5) if name == TA else (3, n)) and len(plan.cells) == 2
    first = plan.out.clone()
    task.reset_idx()
    A = task.num_agents
    torch.cuda.synchronize()
    assert plan.count.tolist() == [1] * n                                        # fill = serve 0, consumed by the reset; serve 1 is waiting
    rows = ball_rows(task, name)
    if name == TA:
        assert np.array_equal(bits(rows), bits(first))                           # the reset from outside a step took the plan's rows too
    else:
        assert np.array_equal(bits(rows[:, 2:5]), bits(first.T.contiguous()))
    # |v| / speed over the configured tilt ranges: >= cos(tilt) cos(tilt_z) (the x component alone), <= sqrt(1 + sin^2 tilt) (TT's form
    # adds a second sine term; the TN / 27-dof form has |v| = speed)
    d = task.env.serve_defaults()
    tmax, tzmax = (np.deg2rad(max(abs(v) for v in d[k])) for k in ("serve_tilt", "serve_tilt_z"))
    lo_f, hi_f = np.cos(tmax) * np.cos(tzmax) - 1e-5, np.sqrt(1.0 + np.sin(tmax) ** 2) + 1e-5
    assert cells[0]["serve_speed"][1] * hi_f < cells[1]["serve_speed"][0] * lo_f  # the two groups cannot be mistaken for each other
    actions = torch.zeros((n * A, task.num_actions), device=DEV)
    resets = torch.zeros(n, dtype=torch.int64, device=DEV)
    for t in range(3 * L_EP + 5):
        before, count = plan.out.clone(), plan.count.clone()
        task.step(actions)
        fired = task.reset_buf[::A] != 0
        resets += fired
        assert torch.equal(plan.count, count + fired.to(torch.int32)), t         # exactly the envs that reset consumed a serve
        if not bool(fired.any()):
            continue
        rows = ball_rows(task, name)[fired]
        want = before[fired] if name == TA else before[:, fired].T.contiguous()
        if name == TA:
            assert np.array_equal(bits(rows), bits(want)), t                     # ball y, z and velocity: the row the buffer held BEFORE the step
        else:
            assert np.array_equal(bits(rows[:, 2:5]), bits(want)), t
        speed = rows[:, 2:5].double().norm(dim=1).cpu().numpy()
        group = (torch.nonzero(fired).flatten() // S).cpu().numpy()
        lo = np.array([cells[g]["serve_speed"][0] for g in group]) * lo_f
        hi = np.array([cells[g]["serve_speed"][1] for g in group]) * hi_f
        assert ((speed >= lo) & (speed <= hi)).all(), (t, speed, group)
        unfired = ~fired
        keep_now, keep_then = (plan.out[unfired], before[unfired]) if name == TA else (plan.out[:, unfired], before[:, unfired])
        assert np.array_equal(bits(keep_now), bits(keep_then)), t
    assert int(resets.min()) >= 2, resets.tolist()                               # every env reset at least twice in the run
    task.clear_serve_plan()
    assert task.env.serve_plan is None and task._serve_plan is None


def test_two_launch_27dof_path_consumes_the_buffer(torch_cuda):
    """TAEnv(fused=False): ppenv_ta_simulate + ppenv_ta_post_physics_step, the latter handed the plan's buffer."""
    torch = torch_cuda
    from isaacgym_amd.tensor_api import TAEnv
    n = 66
    env = TAEnv(n, device=DEV, seed=scene.stream_seed(5, scene.STREAM_ENV), env=dict(episodeLength=6), fused=False)
    plan = env.set_serve_plan(group_cells(TA), paired=True)
    env.reset_idx()
    env.apply_serve_plan(torch.arange(n, device=DEV))
    actions = torch.zeros((n, 27), device=DEV)
    resets = torch.zeros(n, dtype=torch.int64, device=DEV)
    for t in range(20):
        before = plan.out.clone()
        env.step(actions)
        env.apply_serve_plan()
        fired = env.reset_buf != 0
        resets += fired
        assert np.array_equal(bits(env.root_states[:, 2][fired][:, [1, 2, 7, 8, 9]]), bits(before[fired])), t
    assert int(resets.min()) >= 2 and torch.equal(plan.count, (1 + resets).to(torch.int32))
    assert np.array_equal(bits(plan.out[:33, 0:2]), bits(plan.out[33:, 0:2]))     # paired, and the cells differ in speed only: the same ball y, z ...
    assert not bool((plan.out[:33, 2] == plan.out[33:, 2]).any())                 # ... at another speed
    env.close()


# ------------------------------------------------------------------------------------------------------ 8. paired replicas
def run_rows(torch, task, steps):
    A = task.num_agents
    actions = torch.zeros((task.num_envs * A, task.num_actions), device=DEV)
    out = []
    for _ in range(steps):
        task.step(actions)
        out.append((task.obs_buf.clone(), task.rew_buf.clone(), task.reset_buf.clone()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,S", [(TT, 65), (T4, 65), (TA, 64)])
def test_paired_groups_with_equal_cells_are_replicas(torch_cuda, name, S):
    torch = torch_cuda
    n = 2 * S
    steps = 5 * L_EP
    differs = {}
    for paired in (True, False):
        task = make_plain(name, n, 8, episode_length=L_EP)
        task.set_serve_plan([{}, {}], paired=paired)
        task.reset_idx()
        w = S * task.num_agents
        seq = run_rows(torch, task, steps)
        assert any(bool(r.any()) for _, _, r in seq[:L_EP + 1])
        if paired:
            for t, (obs, rew, reset) in enumerate(seq):
                assert np.array_equal(bits(obs[:w]), bits(obs[w:])), (name, t)   # row of env i and of env S + i: bit for bit
                assert np.array_equal(bits(rew[:w]), bits(rew[w:])), (name, t)
                assert torch.equal(reset[:w], reset[w:]), (name, t)
            assert int(task.env.serve_plan.count.min()) >= 3
        differs[paired] = [not np.array_equal(bits(obs[:w]), bits(obs[w:])) for obs, _, _ in seq]
    assert not any(differs[True])
    assert all(differs[False])                                                   # unpaired: different balls from the first serve on


# ------------------------------------------------------------------------------------------------------ 9. clear
def episode_of(task):
    return task.env.episode


@pytest.mark.parametrize("name", [TT, TA])
def test_clear_gives_the_built_in_serves_back(torch_cuda, name):
    torch = torch_cuda
    n = 130
    task, fresh = make_plain(name, n, 13, episode_length=L_EP), make_plain(name, n, 13, episode_length=L_EP)
    episode0 = episode_of(task).clone()
    task.set_serve_plan(group_cells(name), paired=True)
    task.reset_idx()
    run_rows(torch, task, 15)
    task.clear_serve_plan()
    episode_of(task).copy_(episode0)                                             # as Player.end_sweep does: the built-in serves are keyed by it
    task.reset_idx()
    fresh.reset_idx()
    a, b = run_rows(torch, task, 40), run_rows(torch, fresh, 40)
    assert sum(int(r.sum()) for _, _, r in b) >= 3 * n                           # resets, hence built-in serves, happened
    for t in range(40):
        for x, y, what in zip(a[t], b[t], ("obs", "rew", "reset")):
            assert np.array_equal(x.cpu().numpy().view(np.uint8 if what == "reset" else np.uint32).ravel(),
                                  y.cpu().numpy().view(np.uint8 if what == "reset" else np.uint32).ravel()), (name, t, what)
    with pytest.raises(_lib.PPEnvError, match="no plan is set"):
        task.env.apply_serve_plan()


# ------------------------------------------------------------------------------------------------------ 10. captured replay
def test_captured_step_and_apply_replay_like_eager(torch_cuda):
    """One captured env.step + apply_serve_plan pair (one stream, no branches) replayed 40 times equals 40 eager pairs: count[] and the
    buffer live in device memory and the launches take pointers only.  The plan is set BEFORE the capture: the override switch is a by-value
    kernel argument.  Capture succeeding is also the proof that apply_serve_plan does not synchronise."""
    torch = torch_cuda
    from isaacgym_amd.env import PPEnv
    n, K = 300, 40
    cfg = scene.default_task_cfg("TT")
    cfg["env"]["episodeLength"] = 8

    def make():
        env = PPEnv(scene.build_config("TT", cfg=cfg, num_envs=n, seed=scene.stream_seed(4, scene.STREAM_ENV)), device=DEV)
        env.set_serve_plan(group_cells(TT), paired=False)
        env.reset_all()
        env.apply_serve_plan(torch.arange(n, device=DEV))
        return env
    eager, graphed = make(), make()
    actions = torch.zeros(n, 7, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.step(actions)                                                    # warm-up on the capture stream: both code objects are loaded
        graphed.apply_serve_plan()
    torch.cuda.current_stream().wait_stream(side)
    eager.step(actions)
    eager.apply_serve_plan()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step(actions)
        graphed.apply_serve_plan()
    gen = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(K):
        a = torch.rand(n, 7, device=DEV, generator=gen) * 2 - 1
        actions.copy_(a)
        g.replay()
        eager.step(a)
        eager.apply_serve_plan()
    torch.cuda.synchronize()
    assert int(eager.serve_plan.count.min()) >= K // 8                           # every env reset, several times (episodeLength 8)
    for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "ball", "dof_pos", "episode", "serve_override"):
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    assert torch.equal(eager.serve_plan.count, graphed.serve_plan.count)
    eager.close()
    graphed.close()
