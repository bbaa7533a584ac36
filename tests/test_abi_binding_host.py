"""The C ABI is bound once, in isaacgym_amd._lib.load(): every function include/*.h declares has its argtypes set on the default
library and on any library loaded by path.  ctypes hands an unbound function a Python int as a C int: a device pointer would be
truncated without an error, so an unbound entry point is a memory fault waiting for its first caller."""
import glob
import os
import re
import shutil

import pytest

from isaacgym_amd import _lib

DECLARATION = re.compile(r"^(int|size_t|uint32_t|const char\*|void)\s+((?:ppenv|pp_play|pp_serve|pp_render|pp_ta|ppo_meter)_\w+)\(", re.M)


@pytest.fixture(scope="module")
def declared():
    names = []
    for header in sorted(glob.glob(os.path.join(_lib.ROOT, "include", "*.h"))):
        names += [m.group(2) for m in DECLARATION.finditer(open(header).read())]
    assert len(set(names)) >= 106, f"the pattern finds {len(set(names))} declarations in include/*.h; 106 were there when this test was written"
    return sorted(set(names))


def _unbound(L, names):
    return [n for n in names if getattr(L, n).argtypes is None]


def test_every_declared_function_is_bound_on_the_default_library(declared):
    assert _unbound(_lib.lib(), declared) == []


def test_a_library_loaded_by_path_is_fully_bound(declared, tmp_path):
    path = shutil.copy(_lib.LIB_PATH, tmp_path / "libppenv_copy.so")
    L = _lib.load(str(path))
    assert L is not _lib.lib()
    assert _unbound(L, declared) == []


def test_moved_mirrors_keep_their_old_import_paths():
    from isaacgym_amd import play, policy, ppo
    for module, names in ((policy, ("MLPLayer", "MLPDw", "MLPCast")), (ppo, ("PPOLossArgs", "PPOTensor", "PPOAdam")), (play, ("PlayTotals",))):
        for name in names:
            assert getattr(module, name) is getattr(_lib, name), name
    assert play.MAX_AGENTS is _lib.MAX_AGENTS
