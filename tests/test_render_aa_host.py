"""Supersampling in the ray caster without a GPU: render_pixel_aa (isaacgym_amd/csrc/ppenv_render_device.h, compiled by g++:
render_aa_shim_binding) against the one-ray host build — bytewise at samples = 1, by the three-part rule against the box mean of the
s-times larger picture otherwise — the order of the sum, and the refusals of pp_render_rays_aa and Renderer(samples=...)."""
import ctypes as C

import numpy as np
import pytest

import render_aa_shim_binding as ra
import render_shim_binding as rs
from isaacgym_amd import _lib, render
from test_render_host import EINVAL, P, _refused, _valid


@pytest.mark.parametrize("name", ["TT", "T4", "TA"])
def test_one_sample_is_the_plain_picture(name):
    sc, sources, cam = rs.task_scene(rs.TASKS[name])
    assert np.array_equal(ra.shim_render_aa(sc, sources, cam, 64, 48, 1), rs.shim_render(sc, sources, cam, 64, 48)["rgba"])


@pytest.mark.parametrize("name,w,h,s", ra.CASES, ids=ra.CASE_IDS)
def test_supersampled_shim_against_the_box_mean_of_the_larger_plain_picture(name, w, h, s):
    sc, sources, cam, u = ra.undecided_at_rest(name, w, h, s)
    aa = ra.shim_render_aa(sc, sources, cam, w, h, s)[0]
    plain = rs.shim_render(sc, sources, cam, s * w, s * h)["rgba"][0]
    ra.three_part_rule(aa, plain, u, s, f"shim {name} {w}x{h} s={s}")
    assert not np.array_equal(aa, rs.shim_render(sc, sources, cam, w, h)["rgba"][0])          # edges do get in-between colours


def test_the_sum_is_a_binary_tree_over_the_sample_index():
    f = np.float32
    rng = np.random.default_rng(3)
    for n in (1, 4, 16):
        for _ in range(50):
            v = rng.uniform(0, 1, n).astype(f) * f(2.0) ** rng.integers(-12, 1, n).astype(f)     # magnitudes apart: the order shows
            w = list(v)
            while len(w) > 1:
                w = [f(w[k] + w[k + 1]) for k in range(0, len(w), 2)]                          # ((v0 + v1) + (v2 + v3)) + ...
            assert ra.tree_sum(v) == float(w[0])
    v = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 0.0], f)
    assert ra.tree_sum(v) == 1.0 and float(f(f(v[0] + v[3]) + f(v[1] + v[2]))) != 1.0       # another pairing rounds differently


def test_a_supersampled_edge_pixel_is_the_mean_of_its_samples():
    """A sphere's silhouette: inside and outside pixels keep their plain colour, the rim takes colours strictly between."""
    sc = render.Scene("HumanoidPingpongTiltG1")
    sc.source_rows = [1, 1]
    sc.ground_z, sc.checker, sc.diffuse, sc.ambient = -50.0, False, 0.0, 1.0                 # flat colours: albedo or sky
    sc.add(render.RENDER_SPHERE, "s", (1.0, 0.0, 0.0), a=(3.0, 0.0, 1.0), radius=0.25)
    cam = render.Camera((0.0, 0.0, 1.0), (3.0, 0.0, 1.0), fov_deg=30)
    plain = rs.shim_render(sc, [], cam, 33, 25)
    for s in (2, 4):
        aa = ra.shim_render_aa(sc, [], cam, 33, 25, s)[0].astype(int)
        levels = np.unique(aa[..., 0])
        sky_r = int(255 * sc.sky_rgb[0] + 0.5)
        assert levels.min() == sky_r and levels.max() == 255 and len(levels) > 2
        # every red level is sky + (255 - sky) * m / s^2 for a whole number m of samples on the sphere, within the rounding of the channel
        m = (levels - 255 * sc.sky_rgb[0]) / (255 * (1 - sc.sky_rgb[0])) * s * s
        assert np.abs(m - np.round(m)).max() <= 0.51 * s * s / (255 * (1 - sc.sky_rgb[0])) + 1e-6
        big = rs.shim_render(sc, [], cam, 33 * s, 25 * s)["id"][0]
        on = (big == 0).reshape(25, s, 33, s).sum(axis=(1, 3))
        assert np.array_equal(aa[..., 0][on == s * s], np.full((on == s * s).sum(), 255)) and (aa[..., 0][on == 0] == sky_r).all()
    assert set(np.unique(plain["rgba"][0][..., 0])) == {sky_r, 255}


# ---- refusals
class _Task:
    num_envs = 8


@pytest.mark.parametrize("samples", [3, 0, 8, -2, 2.5])
def test_renderer_refuses_samples_other_than_1_2_4(samples):
    with pytest.raises(ValueError, match="1, 2 or 4"):
        render.Renderer(_Task(), samples=samples)
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ra.shim_render_aa(*rs.task_scene(rs.TASKS["TT"]), 8, 8, int(samples) if samples != 2.5 else 3)


@pytest.mark.parametrize("kw", [dict(depth=True), dict(ids=True), dict(depth=True, ids=True)])
def test_renderer_refuses_depth_or_ids_with_supersampling(kw):
    for s in (2, 4):
        with pytest.raises(ValueError, match="samples=1"):
            render.Renderer(_Task(), samples=s, **kw)


def test_entry_refuses_samples_3_and_other_counts():
    sc, prims, cam = _valid()
    for s in (3, 0, -1, 8, 16):
        _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), C.byref(cam), P, P, 1, s, P, None), f"pp_render_rays_aa: samples per axis must be 1, 2 or 4, got {s}")


def test_entry_refuses_null_pointers_and_bad_arguments():
    sc, prims, cam = _valid()
    text = "pp_render_rays_aa: NULL pointer"
    _refused(lambda L: L.pp_render_rays_aa(None, C.byref(cam), P, P, 1, 2, P, None), text)
    _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), None, P, P, 1, 2, P, None), text)
    _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), C.byref(cam), None, P, 1, 2, P, None), text)
    _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), C.byref(cam), P, None, 1, 2, P, None), text)
    _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), C.byref(cam), P, P, 1, 2, None, None), text)
    for count in (0, -1, 17):
        _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), C.byref(cam), P, P, count, 2, P, None),
                 "pp_render_rays_aa: the env selection must have 1 .. 16 entries")
    _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), C.byref(cam), P, P, 1, 4, P + 2, None), "pp_render_rays_aa: rgba must be 4-byte aligned")
    cam.width = 0
    _refused(lambda L: L.pp_render_rays_aa(C.byref(sc), C.byref(cam), P, P, 1, 2, P, None),
             "pp_render_rays_aa: width and height must be positive (at most 16384) and the field of view inside (0, 180) degrees")
    assert EINVAL == -1 and _lib.lib().pp_render_rays_aa.argtypes is not None
