"""ctypes binding of tests/csrc/libppenv_rendershim.so — the ray caster's arithmetic (isaacgym_amd/csrc/ppenv_render_device.h) compiled
for the host, built the way play_shim_binding.lib() builds the episode accounting's — and the cases the host and the GPU tests share.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd import render
from isaacgym_amd._lib import RenderCamera, RenderPosed, RenderPrim, RenderScene

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "render_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_render_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_render.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_rendershim.so")
_lib = None

SIZES = ((64, 48), (72, 40))          # width x height: whole tiles in x and ragged in y, and ragged in both

# The depth bound of the decided pixels.  MEASURED_DEPTH_DEVIATION is the shim's worst relative depth deviation from the fp64
# caster over the host test scenes at both sizes, measured on the CPU (5.29e-07, on the four-kinds scene at 64 x 48; test_render_host
# prints the figure of every scene); the bound is 4 x that, because the GPU's sqrtf and division may round differently and it contracts
# a * b + c.
MEASURED_DEPTH_DEVIATION = 5.3e-7
DEPTH_RTOL = 4 * MEASURED_DEPTH_DEVIATION


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        vp, i32 = C.c_void_p, C.c_int32
        for name, t in (("prim", RenderPrim), ("posed", RenderPosed), ("scene", RenderScene), ("camera", RenderCamera)):
            fn = getattr(L, f"render_shim_sizeof_{name}")
            fn.restype = C.c_size_t
            assert fn() == C.sizeof(t), name
        L.render_shim_pose.restype = L.render_shim_rays.restype = None
        L.render_shim_pose.argtypes = [C.POINTER(RenderScene), C.POINTER(RenderPrim), vp, i32, vp]
        L.render_shim_rays.argtypes = [C.POINTER(RenderScene), C.POINTER(RenderCamera), vp, vp, i32, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_header(sc, sources):
    """pp_render_scene of a render.Scene over host pose arrays [N, rows, 13] float32 (kept alive by the caller)."""
    for s in sources:
        assert s.dtype == np.float32 and s.flags["C_CONTIGUOUS"]
    return sc.header_for(sources[0].shape[0] if sources else 1, [(s.ctypes.data, s.shape[1] * 13, 13, s.shape[1]) for s in sources])


def shim_render(sc, sources, camera, width, height, envs=(0,)):
    """The kernels' arithmetic on the CPU -> dict(posed [E, P, 20] f32, rgba [E, H, W, 4] u8, depth, id, shadow, parity [E, H, W])."""
    L = lib()
    h, cam = host_header(sc, sources), camera.struct(width, height)
    ids_in = np.asarray(envs, np.int32)
    E, P = len(ids_in), len(sc.prims)
    posed = np.zeros((E, max(P, 1), C.sizeof(RenderPosed) // 4), np.float32)
    L.render_shim_pose(C.byref(h), sc.prim_array(), _p(ids_in), E, _p(posed))
    rgba = np.zeros((E, height, width, 4), np.uint8)
    depth = np.zeros((E, height, width), np.float32)
    out = {k: np.zeros((E, height, width), np.int32) for k in ("id", "shadow", "parity")}
    L.render_shim_rays(C.byref(h), C.byref(cam), _p(posed), _p(ids_in), E, _p(rgba), _p(depth), _p(out["id"]), _p(out["shadow"]), _p(out["parity"]))
    return dict(posed=posed, rgba=rgba, depth=depth, **out)


def header_dict(sc):
    """A render.Scene's ground, sky and light for render_reference.cast."""
    return dict(ground_z=sc.ground_z, checker=sc.checker, checker_pitch=sc.checker_pitch, ground_rgb=sc.ground_rgb, sky_rgb=sc.sky_rgb, light=sc.light,
                ambient=sc.ambient, diffuse=sc.diffuse)


def compare(ref, ok, got_id, got_rgba, got_depth, what):
    """The decided-pixel rule: on the pixels `ok` of the fp64 cast `ref`, the same id, colour within +-1 per channel, depth within
    DEPTH_RTOL (both +inf on the sky).  -> worst relative depth deviation found."""
    import render_reference as rr
    assert ok.mean() >= 0.8, f"{what}: {100 * (1 - ok.mean()):.1f} % edge pixels, more than 20 %: move the camera"
    assert np.array_equal(got_id[ok], ref["id"][ok]), f"{what}: {(got_id[ok] != ref['id'][ok]).sum()} decided pixels with another id"
    dc = np.abs(got_rgba[..., :3].astype(np.int64) - rr.rgb8(ref["rgb"]))[ok]
    assert dc.max() <= 1, f"{what}: colour off by {dc.max()} on a decided pixel"
    assert (got_rgba[..., 3] == 255).all()
    sky = ~np.isfinite(ref["depth"])
    assert np.array_equal(np.isposinf(got_depth)[ok], sky[ok]), f"{what}: +inf depth and sky disagree on a decided pixel"
    m = ok & ~sky
    dev = float(np.max(np.abs(got_depth[m] - ref["depth"][m]) / ref["depth"][m])) if m.any() else 0.0
    assert dev <= DEPTH_RTOL, f"{what}: depth deviates by {dev:.3g} relative on a decided pixel, bound {DEPTH_RTOL:.3g}"
    return dev


def task_scene(name):
    """(Scene.from_config(name), its host pose arrays at the reset pose, a side camera)."""
    sc = render.Scene.from_config(name)
    rb, root = sc.rest_states()
    return sc, [rb, root], render.Camera.side_view(sc)


TASKS = {"TT": "HumanoidPingpongTiltG1", "T4": "Humanoid12PingpongTiltG1", "TA": "HumanoidPingpongTiltNESSparse27DOFG1"}
