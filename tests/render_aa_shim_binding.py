"""ctypes binding of tests/csrc/libppenv_renderaashim.so — the ray caster's supersampled pixel (render_pixel_aa of
isaacgym_amd/csrc/ppenv_render_device.h) compiled for the host, built as render_shim_binding builds the one-ray pixel — and the
three-part rule the host and the GPU tests share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

import render_reference as rr
import render_shim_binding as rs
from helpers import build_shim
from isaacgym_amd._lib import RenderCamera, RenderPosed, RenderScene

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "render_aa_shim.cpp")
_LIB = os.path.join(_HERE, "csrc", "libppenv_renderaashim.so")
_lib = None

# (scene, width, height, samples per axis): where the fp64 caster alone leaves at most 20 % of the pixels undecided at the reset pose under
# Camera.side_view (s = 4 at 72 x 40 does not: 21.6 % / 23.5 % for TT / T4)
CASES = (("TT", 64, 48, 2), ("T4", 64, 48, 2), ("TA", 64, 48, 2), ("TT", 72, 40, 2), ("TT", 64, 48, 4))
CASE_IDS = [f"{n}-{w}x{h}-s{s}" for n, w, h, s in CASES]
MAX_UNDECIDED = 0.25
# Each plain sample's byte is within 0.5 of 255 x its float colour and so is the byte of the mean: 1 level; 1e-3 covers the fp32 sum of 16 values.
DECIDED_BOUND = 1 + 1e-3


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, rs._HDRS, ["-ffp-contract=off"])
        vp, i32 = C.c_void_p, C.c_int32
        L.render_aa_shim_rays.argtypes = [C.POINTER(RenderScene), C.POINTER(RenderCamera), vp, vp, i32, i32, vp]
        L.render_aa_shim_tree_sum.restype = C.c_float
        L.render_aa_shim_tree_sum.argtypes = [vp, i32]
        _lib = L
    return _lib


def shim_render_aa(sc, sources, camera, width, height, samples, envs=(0,)):
    """render_pixel_aa on the CPU -> rgba [E, H, W, 4] u8; ValueError for samples the arithmetic refuses."""
    L, R = lib(), rs.lib()
    h, cam = rs.host_header(sc, sources), camera.struct(width, height)
    ids_in = np.asarray(envs, np.int32)
    E, P = len(ids_in), len(sc.prims)
    posed = np.zeros((E, max(P, 1), C.sizeof(RenderPosed) // 4), np.float32)
    R.render_shim_pose(C.byref(h), sc.prim_array(), rs._p(ids_in), E, rs._p(posed))
    rgba = np.zeros((E, height, width, 4), np.uint8)
    if L.render_aa_shim_rays(C.byref(h), C.byref(cam), rs._p(posed), rs._p(ids_in), E, int(samples), rs._p(rgba)) != 0:
        raise ValueError(f"samples per axis must be 1, 2 or 4, got {samples}")
    return rgba


def tree_sum(values):
    v = np.ascontiguousarray(values, np.float32)
    return float(lib().render_aa_shim_tree_sum(rs._p(v), len(v)))


def block_mean(plain, s):
    """[sH, sW, C] uint8 -> [H, W, C] float64: the mean of every s x s block."""
    H, W = plain.shape[0] // s, plain.shape[1] // s
    return plain.astype(np.float64).reshape(H, s, W, s, -1).mean(axis=(1, 3))


def undecided_of(sc, sources, camera, width, height, s, env=0, body_xyz=None):
    """u [H, W]: how many of a pixel's s x s sub-samples rr.decided (fp64) leaves undecided at s width x s height.  body_xyz: where the
    body a follow camera follows is."""
    posed = rr.place(sc.prims, sources, env)
    eye, target = camera.eye_target(body_xyz)
    _, ok = rr.decided(posed, rs.header_dict(sc), eye, target, camera.up, camera.fov_deg, s * width, s * height)
    return (~ok).reshape(height, s, width, s).sum(axis=(1, 3))


_rest = {}


def undecided_at_rest(name, width, height, s):
    """(scene, pose arrays, camera, u) of a task at its reset pose under Camera.side_view: worked out once per case and shared, unchanged,
    by the tests of a process."""
    key = (name, width, height, s)
    if key not in _rest:
        sc, sources, cam = rs.task_scene(rs.TASKS[name])
        u = undecided_of(sc, sources, cam, width, height, s)
        u.setflags(write=False)
        _rest[key] = (sc, sources, cam, u)
    return _rest[key]


def three_part_rule(aa, plain, u, s, what):
    """aa [H, W, 4] uint8 supersampled at W x H; plain [sH, sW, 4] uint8 one ray per pixel at sW x sH; u [H, W] undecided sub-samples.
    (i) decided pixels: |aa - block mean| <= 1 + 1e-3 per channel; (ii) every pixel: <= 1 + 1e-3 + 255 u / s^2; (iii) <= 25 % undecided.
    -> (share of undecided pixels, worst difference on a decided pixel), printed before the assertions."""
    assert aa.shape[:2] == u.shape and plain.shape[:2] == (s * u.shape[0], s * u.shape[1])
    diff = np.abs(aa[..., :3].astype(np.float64) - block_mean(plain[..., :3], s)).max(axis=-1)
    dec = u == 0
    share = float(1.0 - dec.mean())
    worst = float(diff[dec].max())
    over = diff - (DECIDED_BOUND + 255.0 * u / (s * s))
    print(f"{what}: {100 * share:.1f} % undecided pixels, worst difference on a decided pixel {worst:.4f}, worst excess over the bound {over.max():.4f}")
    assert worst <= DECIDED_BOUND, f"{what}: a decided pixel differs from its block mean by {worst}"
    assert (over <= 0).all(), f"{what}: {(over > 0).sum()} pixels exceed 1 + 1e-3 + 255 u / s^2, by up to {over.max()}"
    assert share <= MAX_UNDECIDED, f"{what}: {100 * share:.1f} % undecided pixels, more than 25 %"
    assert (aa[..., 3] == 255).all()
    return share, worst
