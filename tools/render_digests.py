"""Record the bytes of the ray caster's six C entries (include/ppenv_render.h): sha256 of every output of pp_render_pose, pp_render_pose_anchor,
pp_render_rays, pp_render_rays_aa and pp_render_rays_frames on scripted inputs, into tests/golden/render_digests.json.  The entries are driven
directly through _lib: no task, no env kernel, nothing random on the device.  tests/test_render_digests_gpu.py compares against this file.  It
was recorded on one MI355X from the commit BEFORE the ray kernels and the pose kernels were folded into one family each, and is recorded again
only when the caster's arithmetic is changed on purpose.  Needs a GPU.

    python tools/render_digests.py [--out tests/golden/render_digests.json]

Inputs, per scene of render_shim_binding.TASKS: Scene.from_config(name).rest_states() tiled to NUM_ENVS envs, every row's position moved by up
to +-0.3 m and its quaternion perturbed and renormalised in fp32, from np.random.default_rng(SEED + scene + frame) on the host; FRAMES such
sets are the frames.  Selections, picture sizes and cameras: SELECTIONS (the last one reaches the kernels' out-of-range guard from both sides),
SIZES, CAMERAS.  Every output buffer is zeroed before its launch.  The eager entries draw frame 0; pp_render_rays_frames draws all frames in
one launch.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
SEED, NUM_ENVS, FRAMES = 20, 8, 3
SELECTIONS = ((0,), (7, 0, 5), (5, -1, 8, 0))
SIZES = ((33, 17), (16, 16), (1, 1), (72, 40))          # ragged in both axes at every sample count, one tile at one sample, one pixel, several tiles
CAMERAS = ("side", "follow")
SAMPLES = (1, 2, 4)


def pose_frames(sc, seed):
    """-> FRAMES x (rigid_body_states, root_states), float32 [NUM_ENVS, rows, 13] on the host."""
    out = []
    for f in range(FRAMES):
        rng = np.random.default_rng(seed + f)
        pair = []
        for rest in sc.rest_states():
            t = np.tile(rest, (NUM_ENVS, 1, 1)).astype(np.float32)
            t[..., :3] += rng.uniform(-0.3, 0.3, t[..., :3].shape).astype(np.float32)
            q = t[..., 3:7] + rng.uniform(-0.2, 0.2, t[..., 3:7].shape).astype(np.float32)
            t[..., 3:7] = q / np.sqrt((q * q).sum(-1, keepdims=True, dtype=np.float32))
            pair.append(np.ascontiguousarray(t))
        out.append(pair)
    return out


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def scene_entries(torch, L, key, name, seed):
    """Yield (entry key, sha256 hex) of every digest of one scene."""
    from isaacgym_amd import _lib, render
    sc = render.Scene.from_config(name)
    st = _lib.stream(torch.device(DEV))
    P = max(len(sc.prims), 1)
    frames = [[torch.from_numpy(a).to(DEV) for a in pair] for pair in pose_frames(sc, seed)]
    headers = [sc.header_for(NUM_ENVS, [(t.data_ptr(), t.stride(0), t.stride(1), t.shape[1]) for t in pair]) for pair in frames]
    prims_dev = torch.zeros(P * C.sizeof(_lib.RenderPrim), dtype=torch.uint8, device=DEV)
    prims = sc.prim_array()
    _lib.check(L.pp_render_scene_upload(C.byref(headers[0]), prims, prims_dev.data_ptr(), st), L)
    torch.cuda.synchronize()
    cams = dict(side=render.Camera.side_view(sc), follow=render.Camera.follow_root(sc))
    for sel in SELECTIONS:
        E, tag = len(sel), f"{key}/envs{','.join(str(e) for e in sel)}"
        ids = torch.tensor(sel, dtype=torch.int32, device=DEV)
        posed = torch.zeros((FRAMES, E, P, render.POSED_WORDS), dtype=torch.int32, device=DEV)
        for f, h in enumerate(headers):
            _lib.check(L.pp_render_pose(C.byref(h), prims_dev.data_ptr(), ids.data_ptr(), E, posed[f].data_ptr(), st), L)
            yield f"{tag}/pose/frame{f}/posed", sha(posed[f])
        anchor = torch.zeros((FRAMES, E, 4), dtype=torch.float32, device=DEV)
        for row in (-1, 0):                                                               # no anchor body; the first humanoid's root (kept for the casts below)
            again = torch.zeros_like(posed)
            anchor.zero_()
            for f, h in enumerate(headers):
                _lib.check(L.pp_render_pose_anchor(C.byref(h), prims_dev.data_ptr(), ids.data_ptr(), E, render.SRC_ROOT, row, again[f].data_ptr(),
                                                   anchor[f].data_ptr(), st), L)
                yield f"{tag}/pose_anchor/row{row}/frame{f}/posed", sha(again[f])
                yield f"{tag}/pose_anchor/row{row}/frame{f}/anchor", sha(anchor[f])
        h = headers[0]
        for w, hh in SIZES:
            for cname in CAMERAS:
                cam = cams[cname].struct(w, hh)
                what = f"{tag}/{w}x{hh}/{cname}"
                rgba = torch.zeros((FRAMES, E, hh, w, 4), dtype=torch.uint8, device=DEV)
                depth = torch.zeros((E, hh, w), dtype=torch.float32, device=DEV)
                pid = torch.zeros((E, hh, w), dtype=torch.int32, device=DEV)
                _lib.check(L.pp_render_rays(C.byref(h), C.byref(cam), posed[0].data_ptr(), ids.data_ptr(), E, rgba[0].data_ptr(), depth.data_ptr(),
                                            pid.data_ptr(), st), L)
                yield f"{what}/rays/rgba", sha(rgba[0])
                yield f"{what}/rays/depth", sha(depth)
                yield f"{what}/rays/ids", sha(pid)
                rgba.zero_()
                _lib.check(L.pp_render_rays(C.byref(h), C.byref(cam), posed[0].data_ptr(), ids.data_ptr(), E, rgba[0].data_ptr(), None, None, st), L)
                yield f"{what}/rays_null/rgba", sha(rgba[0])
                for s in SAMPLES:
                    rgba.zero_()
                    _lib.check(L.pp_render_rays_aa(C.byref(h), C.byref(cam), posed[0].data_ptr(), ids.data_ptr(), E, s, rgba[0].data_ptr(), st), L)
                    yield f"{what}/rays_aa{s}/rgba", sha(rgba[0])
                for s in SAMPLES:
                    for anc in ((anchor, None) if cname == "side" else (anchor,)):      # a fixed camera reads no anchor: given and NULL
                        rgba.zero_()
                        _lib.check(L.pp_render_rays_frames(C.byref(h), C.byref(cam), posed.data_ptr(), _lib.ptr(anc), FRAMES, E, s, rgba.data_ptr(), st), L)
                        yield f"{what}/rays_frames{s}{'' if anc is not None else '_null_anchor'}/rgba", sha(rgba)
    torch.cuda.synchronize()
    del prims


def entries(torch):
    """Yield (entry key, sha256 hex) of every digest, in a fixed order."""
    from isaacgym_amd import _lib
    from render_shim_binding import TASKS
    L = _lib.lib()
    for i, (key, name) in enumerate(TASKS.items()):
        yield from scene_entries(torch, L, key, name, SEED + 100 * i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "render_digests.json"))
    args = ap.parse_args()
    import torch
    hipcc = subprocess.run([os.environ.get("HIPCC", "hipcc"), "--version"], capture_output=True, text=True).stdout.strip()
    recorded = dict(entries(torch))
    with open(args.out, "w") as fh:
        json.dump(dict(made_with=dict(hipcc=hipcc, numpy=np.__version__, torch=torch.__version__), seed=SEED, num_envs=NUM_ENVS, frames=FRAMES,
                       entries=recorded), fh, indent=0)
        fh.write("\n")
    print(f"wrote {len(recorded)} digests to {args.out}")


if __name__ == "__main__":
    main()
