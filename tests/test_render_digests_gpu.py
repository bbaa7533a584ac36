"""The ray caster's bytes on the MI355X: every output of the six C entries of include/ppenv_render.h on the scripted inputs of
tools/render_digests.py has the sha256 recorded in tests/golden/render_digests.json.  The file was recorded from the commit that still had
three ray kernels (render_rays_kernel, render_rays_aa_kernel, render_rays_frames_kernel) and two pose kernels; render_rays_kernel<S> and
render_pose_kernel have to give those bytes.  The other GPU tests compare the entries with each other and with the host build to a tolerance;
this one holds the arithmetic itself.  A digest that differs means a pixel, a posed word or an anchor moved: the file stays.  Need a real MI355X."""
import importlib.util
import json
import os

import pytest

from render_shim_binding import TASKS

pytestmark = pytest.mark.gpu

_TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def digests():
    """(tools/render_digests.py as a module, the recorded entries)."""
    spec = importlib.util.spec_from_file_location("render_digests", os.path.join(_TESTS, "..", "tools", "render_digests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(_TESTS, "golden", "render_digests.json")) as fh:
        recorded = json.load(fh)
    assert (recorded["seed"], recorded["num_envs"], recorded["frames"]) == (tool.SEED, tool.NUM_ENVS, tool.FRAMES)
    return tool, recorded["entries"]


@pytest.mark.parametrize("key", list(TASKS))
def test_every_entry_gives_the_recorded_bytes(digests, key):
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from isaacgym_amd import _lib
    tool, recorded = digests
    want = {k: v for k, v in recorded.items() if k.startswith(key + "/")}
    got = dict(tool.scene_entries(torch, _lib.lib(), key, TASKS[key], tool.SEED + 100 * list(TASKS).index(key)))
    assert set(got) == set(want) and len(want) > 300, f"{key}: the tool's entries and the recorded ones are not the same set"
    wrong = [k for k in got if got[k] != want[k]]                                         # scene/envs<selection>/<width>x<height>/<camera>/<entry>/<output>
    assert not wrong, f"{len(wrong)} of {len(got)} outputs differ from the recorded bytes: {wrong[:12]}"
