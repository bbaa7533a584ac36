"""The 27-dof task's outcome counts (include/ppenv_ta_outcome.h) without a GPU: the ctypes mirror against the header, the new entries' NULL
refusals, the kernels' arithmetic compiled for the host (tests/csrc/ta_outcome_shim.cpp) against numpy popcounts, the latch rule, and
the windows of tests/golden/post_physics_TA.npz under the unmodified oracle."""
import ctypes as C

import numpy as np
import pytest

import ta_outcome_shim_binding as B
from isaacgym_amd import _lib
from isaacgym_amd._lib import TAOutcome

EINVAL = -1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_mirror_equals_the_header():
    L = B.lib()
    off = (C.c_size_t * 6)()
    L.ta_outcome_shim_offsets(C.byref(off))
    assert list(off) == [0, 8, 16, 56, 64, 104]
    o = TAOutcome
    assert [o.windows.offset, o.envs.offset, o.count.offset, o.last_envs.offset, o.last.offset, o.reserved.offset] == list(off)
    assert C.sizeof(o) == L.ta_outcome_shim_sizeof() == 128
    assert _lib.TA_OUTCOME_NAMES == ("closer", "hit_paddle", "cross_net", "hit_table", "fall_down")


@pytest.mark.parametrize("name, text", [
    ("pp_ta_sim_set_outcome", "pp_ta_sim_set_outcome: NULL handle"),
    ("pp_ta_post_physics_step_outcome", "pp_ta_post_physics_step_outcome: NULL argument or num_envs <= 0"),
    ("pp_ta_outcome_latch", "pp_ta_outcome_latch: NULL pointer, a struct that is not 8-byte aligned, or games_num < 1"),
])
def test_null_is_refused_with_the_pinned_code_and_text(name, text):
    L = _lib.lib()
    assert L.ppenv_gae(*([None] * 2 + [0, 0, None, 0, 0, 0.0, 0.0, 0.0, None, None, None])) == EINVAL      # another text in ppenv_last_error()
    assert L.ppenv_last_error().decode() != text
    fn = getattr(L, name)
    args = [None if issubclass(t, (C.c_void_p, C._Pointer)) else 0 for t in fn.argtypes]
    assert fn(*args) == EINVAL
    assert L.ppenv_last_error().decode() == text


def test_the_old_entry_keeps_its_text():
    L = _lib.lib()
    fn = L.ppenv_ta_post_physics_step
    assert fn(*([None] * len(fn.argtypes))) == EINVAL
    assert L.ppenv_last_error().decode() == "ppenv_ta_post_physics_step: NULL argument or num_envs <= 0"


@pytest.mark.parametrize("n", [0, 1, 64, 130])
def test_shim_sums_equal_numpy_popcounts(n):
    L = B.lib()
    rng = np.random.default_rng(100 + n)
    words = np.zeros(B.WORDS, np.uint64)
    want = words.copy()
    for window in range(3):
        flags = B.random_flags(n, rng)
        before = flags.copy()
        L.ta_outcome_shim_clear(n, _p(flags), 0, _p(words))                   # nobody reset: nothing changes
        np.testing.assert_array_equal(flags, before)
        np.testing.assert_array_equal(words, want)
        L.ta_outcome_shim_clear(n, _p(flags), 1, _p(words))
        B.add_window(want, n, B.popcounts(before))
        np.testing.assert_array_equal(words, want)
        np.testing.assert_array_equal(flags, before & ~np.uint32(B.COUNT_MASK))       # the sticky bits stay
    assert int(words[0]) == 3 and int(words[1]) == 3 * n
    np.testing.assert_array_equal(words[13:], 0)
    flags = B.random_flags(n, rng)
    before = flags.copy()
    L.ta_outcome_shim_clear(n, _p(flags), 1, None)                            # off: the clear alone
    np.testing.assert_array_equal(flags, before & ~np.uint32(B.COUNT_MASK))
    np.testing.assert_array_equal(words, want)


def test_popcounts_order_is_the_bit_order():
    flags = np.array([16, 16 | 32, 64, 128 | 1, 256 | 2, 256, 15], np.uint32)
    np.testing.assert_array_equal(B.popcounts(flags), [2, 1, 1, 1, 2])
    L = B.lib()
    words = np.zeros(B.WORDS, np.uint64)
    L.ta_outcome_shim_clear(flags.size, _p(flags), 1, _p(words))
    np.testing.assert_array_equal(words[2:7], [2, 1, 1, 1, 2])
    np.testing.assert_array_equal(words[8:13], [2, 1, 1, 1, 2])
    assert int(words[7]) == 7


@pytest.mark.parametrize("games, games_num, copies", [(0, 1, True), (9, 10, True), (10, 10, False), (11, 10, False)])
def test_latch_copies_only_while_the_totals_are_not_frozen(games, games_num, copies):
    L = B.lib()
    rng = np.random.default_rng(7)
    live = rng.integers(0, 2 ** 63, B.WORDS, dtype=np.uint64)
    latched = rng.integers(0, 2 ** 63, B.WORDS, dtype=np.uint64)
    before = latched.copy()
    L.ta_outcome_shim_latch(_p(live), games, games_num, _p(latched))
    assert latched.tobytes() == (live if copies else before).tobytes()


def test_golden_windows_under_the_unmodified_oracle(oracle_lib):
    from test_ta_golden import load
    e = B.golden_expectation(oracle_lib)
    g = load()
    windows = np.nonzero(e["resets"])[0]
    assert windows.tolist() == [12, 25] and e["resets"][windows].tolist() == [e["n"], e["n"]] == [32, 32]
    # what the reference's own run left one step earlier: a lower bound of the head-counts its prints showed
    left = [B.popcounts(g["out_flags"][t - 1]) for t in windows]
    assert [v.tolist() for v in left] == [[25, 15, 1, 3, 15], [23, 15, 4, 0, 22]]
    for t, lo in zip(windows, left):
        assert (e["preclear"][t] >= lo).all(), (t, e["preclear"][t], lo)
    assert (e["preclear"][windows].max(axis=0) > 0).all()
    last = e["structs"][-1]
    assert int(last[0]) == 2 and int(last[1]) == 64
    np.testing.assert_array_equal(last[2:7], e["preclear"][12] + e["preclear"][25])
    np.testing.assert_array_equal(last[8:13], e["preclear"][25])
    assert (g["out_flags"][windows] & B.COUNT_MASK == 0).all()                # the step that resets is the step that clears
