"""Supersampling in the ray caster on the MI355X (pp_render_rays_aa, Renderer(samples=...)): one sample is pp_render_rays byte for byte,
2 x 2 and 4 x 4 samples follow the three-part rule (render_aa_shim_binding) against the box mean of the s-times larger one-ray picture,
repeatability, env selections, a captured graph, the follow camera, and rendering as a read-only observer.  8 envs.  Need a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import render_aa_shim_binding as ra
import render_shim_binding as rs
from test_render_gpu import DEV, SELECTIONS, host_sources, make, random_steps, snapshot

pytestmark = pytest.mark.gpu

TT, TA, T4 = rs.TASKS["TT"], rs.TASKS["TA"], rs.TASKS["T4"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


@pytest.mark.parametrize("sel", [SELECTIONS[0], SELECTIONS[2]], ids=["one", "sixteen"])
def test_one_sample_is_pp_render_rays_byte_for_byte(torch_cuda, sel):
    torch = torch_cuda
    from isaacgym_amd import _lib, render
    task = make(TT)
    random_steps(torch, task, 12)
    r = render.Renderer(task, envs=sel, width=72, height=40)
    plain = r.render().clone()
    out = torch.zeros_like(plain)
    sc = r.scene
    _lib.check(r.L.pp_render_rays_aa(C.byref(sc.header), C.byref(r._cam), r.posed.data_ptr(), r.env_ids.data_ptr(), len(sel), 1, out.data_ptr(),
                                     _lib.stream(DEV)), r.L)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and int(plain[..., :3].max()) > 0
    if len(sel) > 1:
        assert not torch.equal(plain[0], plain[1])


@pytest.mark.parametrize("name,w,h,s", ra.CASES, ids=ra.CASE_IDS)
def test_supersampled_kernel_against_the_box_mean_of_the_larger_plain_picture(torch_cuda, name, w, h, s):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make(rs.TASKS[name])                                                        # fresh, not stepped: the reset pose
    big = render.Renderer(task, envs=[0], width=s * w, height=s * h)
    plain = big.render().cpu().numpy()[0]
    r = render.Renderer(task, envs=[0], width=w, height=h, samples=s)
    aa = r.render().cpu().numpy()[0]
    u = ra.undecided_of(r.scene, host_sources(r), r.camera, w, h, s)
    ra.three_part_rule(aa, plain, u, s, f"kernel {name} {w}x{h} s={s}")
    small = render.Renderer(task, envs=[0], width=w, height=h).render().cpu().numpy()[0]
    assert not np.array_equal(aa, small)


@pytest.mark.parametrize("s", [2, 4])
def test_two_renders_are_bitwise_equal_and_an_env_alone_is_the_env_among_others(torch_cuda, s):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make(T4)
    random_steps(torch, task, 12)
    w, h = 72, 40
    sel = SELECTIONS[2]
    r = render.Renderer(task, envs=sel, width=w, height=h, samples=s)
    first = r.render().clone()
    assert torch.equal(r.render(), first)
    other = torch.zeros_like(first)
    assert torch.equal(r.render(out=other), first)
    alone = {}
    for e in sorted(set(sel)):
        alone[e] = render.Renderer(task, envs=[e], width=w, height=h, samples=s).render().clone()
    for k, e in enumerate(sel):
        assert torch.equal(first[k], alone[e][0]), f"env {e} at position {k} of {sel} differs from the env drawn alone"
    assert not torch.equal(alone[0], alone[5])                                         # the envs do differ after 12 random steps


@pytest.mark.parametrize("name,s", [(TT, 2), (TA, 4)], ids=["TT-s2", "TA-s4"])
def test_supersampled_render_replays_in_a_captured_graph(torch_cuda, name, s):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make(name)
    random_steps(torch, task, 3)
    r = render.Renderer(task, envs=[0, 6], width=72, height=40, samples=s)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        r.render()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r.render()
    before = r.rgba.clone()
    random_steps(torch, task, 4, seed=12)
    g.replay()
    torch.cuda.synchronize()
    replayed = r.rgba.clone()
    eager = r.render().clone()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, before)


def test_the_follow_camera_with_two_by_two_samples(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import render
    task = make(TA)
    w, h, s, env = 64, 48, 2, 1
    r = render.Renderer(task, envs=[env], width=w, height=h, samples=s)
    big = render.Renderer(task, envs=[env], width=s * w, height=s * h)
    # the looking-down follow camera of test_the_follow_cam_keeps_the_root_on_the_centre_column (no horizon through so small a picture)
    cam = render.Camera((0.0, -3.0, 3.0), (0.0, 0.0, 0.6), follow=render.Camera.follow_root(r.scene).follow)
    r.set_camera(cam)
    big.set_camera(cam)
    pictures = []
    for steps in (0, 20):
        random_steps(torch, task, steps, seed=steps + 1)
        aa, plain = r.render().cpu().numpy()[0], big.render().cpu().numpy()[0]
        sources = host_sources(r)
        root = sources[1][env, 0, :3].astype(np.float64)
        u = ra.undecided_of(r.scene, sources, cam, w, h, s, env=env, body_xyz=root)
        ra.three_part_rule(aa, plain, u, s, f"follow camera after {steps} steps")
        pictures.append((aa, root))
    assert np.abs(pictures[1][1][:2] - pictures[0][1][:2]).max() > 1e-3, "the root did not move: the test shows nothing"


@pytest.mark.parametrize("name", [TT, T4, TA], ids=["TT", "T4", "TA"])
def test_supersampled_rendering_changes_no_env_state(torch_cuda, name):
    torch = torch_cuda
    from isaacgym_amd import render
    snaps = []
    for draw in (False, True):
        task = make(name, episode_length=12)                                           # resets happen within the 16 steps
        r = render.Renderer(task, envs=[0, 3, 7], width=64, height=48, samples=4) if draw else None
        gen = torch.Generator(device=DEV).manual_seed(5)
        for _ in range(16):
            task.step(torch.rand((task.num_envs * task.num_agents, task.num_actions), device=DEV, generator=gen) * 2 - 1)
            if draw:
                r.render()
        snaps.append(snapshot(torch, task))
    assert len(snaps[0]) == len(snaps[1])
    for a, b in zip(*snaps):
        assert a.tobytes() == b.tobytes()
