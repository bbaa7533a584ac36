"""ctypes binding of tests/csrc/libppenv_taoutcomeshim.so — the outcome-count arithmetic of the HIP kernels
(isaacgym_amd/csrc/ppenv_ta_outcome_device.h) compiled for the host, built the way play_shim_binding.lib() builds the episode accounting's —
and the numpy expectations the host and the GPU tests of the outcome counts share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd._lib import TAOutcome

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "ta_outcome_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_ta_outcome_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_ta_outcome.h"), os.path.join(_HERE, "..", "include", "ppenv_play.h"),
         os.path.join(_HERE, "..", "include", "ppenv.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_taoutcomeshim.so")
_lib = None

COUNT_BITS = (16, 32, 64, 128, 256)            # closer, hit_paddle, cross_net, hit_table, fall_down (PPENV_TA_COUNT_*)
COUNT_MASK, STICKY_MASK = 0x1F0, 0xF
WORDS = 16                                     # pp_ta_outcome as uint64 words


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, [])
        L.ta_outcome_shim_sizeof.restype = C.c_size_t
        L.ta_outcome_shim_clear.restype = L.ta_outcome_shim_latch.restype = None
        L.ta_outcome_shim_clear.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.ta_outcome_shim_latch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.ta_outcome_shim_offsets.restype = None
        L.ta_outcome_shim_offsets.argtypes = [C.POINTER(C.c_size_t * 6)]
        assert L.ta_outcome_shim_sizeof() == C.sizeof(TAOutcome) == 128
        _lib = L
    return _lib


def popcounts(flags):
    """The five head-counts of a flag vector, in the struct's order — numpy, independent of the kernel text."""
    f = np.asarray(flags).astype(np.uint32)
    return np.array([int(np.count_nonzero(f & b)) for b in COUNT_BITS], np.uint64)


def add_window(words, n, counts):
    """What one window does to the struct (a uint64 [16] array, changed in place): the header's rule restated in numpy."""
    words[0] += np.uint64(1)
    words[1] += np.uint64(n)
    words[2:7] += counts.astype(np.uint64)
    words[7] = np.uint64(n)
    words[8:13] = counts.astype(np.uint64)
    return words


def random_flags(n, rng):
    """n flag words with the five count bits and the four sticky bits set at random."""
    return rng.integers(0, 0x200, n, dtype=np.uint32)


# ---- the golden fixture's windows, from the UNMODIFIED oracle (ppo_ta_post_physics_step): shared by the host and the GPU test
RAISED = 1 << 30                               # a max_episode_length under which nobody resets
_golden = None


def golden_expectation(oracle_lib):
    """tests/golden/post_physics_TA.npz stepped by the oracle with the flags carried step to step, as test_ta_golden.py does.  The count bits do
    not depend on the reset decision and a reset clears only the sticky bits, so the bits "right before the clear" of step t are what the same
    step leaves when max_episode_length is raised so that nobody resets: the oracle is called twice per step, on copies with it raised and
    for real.  -> dict(resets [T] envs that reset, preclear [T, 5] head-counts of the raised call, structs [T, 16] the struct after each step)."""
    global _golden
    if _golden is None:
        import copy
        from test_ta_golden import load, params_for
        g = load()
        p = params_for(g)
        hi = copy.copy(p)
        hi.max_episode_length = RAISED
        T, n = g["out_rew"].shape
        irb = np.ascontiguousarray(np.broadcast_to(g["initial_bodies42"], (n, 42, 13)), np.float32)
        flags, episode, progress = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int64)
        resets, preclear, structs, words = [], [], [], np.zeros(WORDS, np.uint64)
        for t in range(T):
            args = lambda: (np.ascontiguousarray(g["in_bodies42"][t]), irb, g["in_root"][t].copy(), g["in_dof"][t].copy(), g["in_dof_force"][t].copy(),
                            g["in_pre_vx"][t].copy(), np.nan_to_num(g["reset_override"][t]))
            f_hi, e_hi, p_hi = flags.copy(), episode.copy(), progress.copy()
            _, _, r_hi = oracle_lib.ta_post_physics_step(hi, *args(), f_hi, e_hi, p_hi)
            assert not r_hi.any()
            _, _, reset = oracle_lib.ta_post_physics_step(p, *args(), flags, episode, progress)
            np.testing.assert_array_equal(flags, g["out_flags"][t])
            resets.append(int(np.count_nonzero(reset)))
            preclear.append(popcounts(f_hi))
            if reset.any():
                add_window(words, n, preclear[-1])
            structs.append(words.copy())
        _golden = dict(resets=np.array(resets), preclear=np.array(preclear), structs=np.array(structs), n=n, T=T)
    return _golden
