"""The serve curriculum (include/ppenv_serve_curric.h) without a GPU.  The rule is this project's own — no oracle pins it — so it is checked
against itself restated twice: the host build of the kernels' per-env and per-bin code (tests/csrc/serve_curric_shim.cpp) against numpy
written from the header's words (serve_curric_shim_binding.NumpyCurric), every word equal; then the properties of the table, the refusals of
the real library's host-side validation, the ctypes mirrors, the grid cutting and the CLI parser."""
import ctypes as C
import math

import numpy as np
import pytest

import serve_curric_shim_binding as scb
from isaacgym_amd import _lib, curriculum, scene
from test_serve_plan_host import ubits

SOA, AOS = _lib.SERVE_LAYOUT_SOA3, _lib.SERVE_LAYOUT_AOS5
U32, F32, I64 = np.uint32, np.float32, np.int64
ONE = 1 << 24
EINVAL = -1
SEED = scene.stream_seed(42, scene.STREAM_SERVES)


def pair(n, bins, form, layout, **kw):
    return scb.HostCurric(n, bins, form, layout, **kw), scb.NumpyCurric(n, bins, form, layout, **kw)


# ------------------------------------------------------------------------------------------------------ 1. the mirrors and the draw
def test_ctypes_mirrors_match_the_headers_layout():
    L = scb.lib()
    o = (C.c_size_t * 22)()
    L.curric_shim_layout(o)
    cur, st = _lib.ServeCurric, _lib.ServeCurricState
    want = [C.sizeof(cur)] + [getattr(cur, name).offset for name, _ in cur._fields_] + [C.sizeof(st)] + [getattr(st, name).offset for name, _ in st._fields_]
    assert list(o) == want and C.sizeof(cur) == 56 and C.sizeof(st) == 64
    k = (C.c_int64 * 5)()
    L.curric_shim_consts(k)
    assert list(k) == [_lib.CURRIC_MAX_BINS, _lib.CURRIC_MAX_POWER, 5, _lib.CURRIC_FOLD_CHUNK, _lib.CURRIC_DROPPED] == [256, 4, 5, scb.CHUNK, scb.DROPPED]


def test_u24_is_the_integer_rng_uniform_scales():
    L = scb.lib()
    rng = np.random.default_rng(0)
    for seed, gid, j in zip(rng.integers(0, 2 ** 63, 500), rng.integers(0, 2 ** 32, 500), rng.integers(0, 2 ** 32, 500)):
        u = L.curric_shim_u24(int(seed), int(gid), int(j))
        assert 0 <= u < ONE and F32(u) * F32(1.0 / 16777216.0) == F32(L.curric_shim_uniform(int(seed), int(gid), int(j)))
        assert u == int(ubits(int(seed), int(gid), int(j), 5)[0])


def test_bin_is_the_count_of_entries_at_or_below_the_draw():
    L = scb.lib()
    rng = np.random.default_rng(1)
    for B in (1, 2, 3, 7, 256):
        cdf = np.sort(rng.integers(0, ONE, B)).astype(U32)
        cdf[B // 2:B // 2 + 2] = cdf[B // 2]                                      # an empty interval
        cdf[-1] = ONE
        probes = np.concatenate([rng.integers(0, ONE, 200), cdf[:-1].astype(I64), cdf[:-1].astype(I64) - 1, [0, ONE - 1]]).clip(0, ONE - 1)
        for u in probes:
            assert L.curric_shim_bin(cdf.ctypes.data, B, int(u)) == int((cdf[:B - 1] <= u).sum())


def test_q_truncates_and_drops():
    L = scb.lib()
    xs = np.array([0.0, -0.0, 1.5, -1.5, 1e-6, -1e-6, 123.456, -2147483648.0, 2147483648.0, 2147483904.0, -2147483904.0, np.inf, -np.inf, np.nan, 3e38], F32)
    got = np.array([L.curric_shim_q(float(x)) for x in xs], I64)
    assert np.array_equal(got, scb.np_q(xs))
    assert got[2] == 98304 and got[3] == -98304 and got[4] == 0 and got[5] == 0                # truncation, towards zero
    assert got[7] == -(2 ** 47) and got[8] == 2 ** 47 and (got[9:] == scb.DROPPED).all()


# ------------------------------------------------------------------------------------------------------ 2. fill
@pytest.mark.parametrize("B", [1, 3, 256])
def test_fill(B):
    h, ref = pair(97, scb.grid_bins(B), scene.VARIANT_TN, AOS, seed=SEED, env_id_offset=3)
    assert not scb.same_words(h.words(), ref.words())
    assert np.array_equal(h.cdf, [((b + 1) << 24) // B for b in range(B)]) and h.cdf[-1] == ONE
    assert (h.cur_bin == -1).all() and (h.ret == 0).all() and (h.count == 0).all()
    assert h.next_bin.min() >= 0 and h.next_bin.max() < B
    if B == 3:
        assert set(h.next_bin.tolist()) == {0, 1, 2}
        speed = np.linalg.norm(h.out[:, 2:5].astype(np.float64), axis=1)          # the TN form: |v| = speed, inside the bin's interval
        lo = np.array([h.cells[b]["serve_speed"][0] for b in h.next_bin])
        hi = np.array([h.cells[b]["serve_speed"][1] for b in h.next_bin])
        assert ((speed >= lo - 1e-4) & (speed <= hi + 1e-4)).all()
    # a refill keeps the counts and redraws from them
    h.count[:] = np.arange(97) % 5
    ref.count[:] = h.count
    h.fill()
    ref.fill()
    assert not scb.same_words(h.words(), ref.words())


# ------------------------------------------------------------------------------------------------------ 3. step, fold, update together
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("layout", [SOA, AOS], ids=["soa3", "aos5"])
@pytest.mark.parametrize("n", [1, 63, 300])
def test_step_over_40_steps(n, layout, A):
    form = scene.VARIANT_TN if layout == AOS else (scene.VARIANT_T4 if A == 2 else scene.VARIANT_TT)
    kw = dict(reset_rows=A, num_agents=A, seed=SEED, env_id_offset=11, power=2, mix=0.1, alpha=0.3)
    h, ref = pair(n, scb.grid_bins(3), form, layout, **kw)
    rew, reset = scb.scripted(40, n, A, A)
    H = 8
    fb = [np.full((H, n), -1, np.int32) for _ in range(2)]
    fq = [np.zeros((H, n), I64) for _ in range(2)]
    first_game, staged_games = np.ones(n, bool), 0
    for t in range(40):
        r = t % H
        before, cur_before = h.words(), h.cur_bin.copy()
        for k, c in enumerate((h, ref)):
            c.step(rew[t], reset[t], fb[k][r], fq[k][r])
        assert not scb.same_words(h.words(), ref.words()), (t, scb.same_words(h.words(), ref.words()))
        assert np.array_equal(fb[0][r], fb[1][r]) and np.array_equal(fq[0][r], fq[1][r]), t
        fired = reset[t][::A] != 0
        after = h.words()
        out_b, out_a = (before["out"][:, ~fired], after["out"][:, ~fired]) if layout == SOA else (before["out"][~fired], after["out"][~fired])
        assert np.array_equal(out_b, out_a), t                                   # a non-resetting env's row is untouched, bit for bit
        for name in ("count", "next_bin", "cur_bin"):
            assert np.array_equal(before[name][~fired], after[name][~fired]), (t, name)
        assert np.array_equal(after["count"][fired], before["count"][fired] + 1)
        assert (fb[0][r][~fired] == -1).all() and np.array_equal(fb[0][r][fired], cur_before[fired])
        assert (fb[0][r][fired & first_game] == -1).all()                        # the game running at installation is not counted
        assert (fb[0][r][fired & ~first_game] >= 0).all()
        staged_games += int((fb[0][r] >= 0).sum())
        first_game &= ~fired
        if t == 6:
            assert fired.all()
        if t == 7:
            assert not fired.any() and (fb[0][r] == -1).all()
        if r == H - 1:
            tots = [c.fold(fb[k], fq[k]) for k, c in enumerate((h, ref))]
            assert np.array_equal(tots[0], tots[1])
            for c, tot in zip((h, ref), tots):
                c.update(tot)
            assert not scb.same_words(h.words(), ref.words()), (t, "update")
            assert (np.diff(h.cdf.astype(I64)) >= 0).all() and h.cdf[-1] == ONE
    assert int(h.games.sum() + h.dropped.sum()) == staged_games > 0
    if n >= 4:
        assert int(h.dropped.sum()) >= 1                                         # inf, nan and beyond 2^31: counted apart, never in a mean
    assert np.isfinite(h.mean).all()


def test_fold_one_bin_no_bin_and_more_than_one_chunk():
    h, ref = pair(5, scb.grid_bins(3), scene.VARIANT_TT, SOA, seed=SEED)
    n, H = 5, 4
    fin_bin, fin_q = np.full((H, n), -1, np.int32), np.zeros((H, n), I64)
    assert not h.fold(fin_bin, fin_q).any() and not ref.fold(fin_bin, fin_q).any()             # no env finished
    fin_bin[2], fin_q[2] = 1, [5, -7, 1 << 40, scb.DROPPED, -(1 << 40)]                          # all envs, one bin, one step
    want = np.zeros((3, 3), I64)
    want[:, 1] = [4, -2, 1]
    assert np.array_equal(h.fold(fin_bin, fin_q), want) and np.array_equal(ref.fold(fin_bin, fin_q), want)
    rng = np.random.default_rng(3)
    count = 2 * scb.CHUNK + 1234                                                               # three chunks, the last one ragged
    big_bin = rng.integers(-1, 256, count).astype(np.int32)
    big_q = rng.integers(-2 ** 47, 2 ** 47, count).astype(I64)
    big_q[rng.random(count) < 0.01] = scb.DROPPED
    h256, ref256 = pair(2, scb.grid_bins(256), scene.VARIANT_TT, SOA, seed=SEED)
    tot = h256.fold(big_bin, big_q)
    assert np.array_equal(tot, ref256.fold(big_bin, big_q)) and tot[0].sum() + tot[2].sum() == (big_bin >= 0).sum()


# ------------------------------------------------------------------------------------------------------ 4. the table
def totals(B, games):
    """tot for {bin: (n, mean return)}"""
    tot = np.zeros((3, B), I64)
    for b, (n, mean) in games.items():
        tot[0, b], tot[1, b] = n, int(round(mean * 65536.0)) * n
    return tot


@pytest.mark.parametrize("power, mix", [(0, 0.25), (3, 1.0), (0, 0.0)])
@pytest.mark.parametrize("B", [1, 3, 7, 256])
def test_power_0_or_mix_1_is_uniform(B, power, mix):
    h, ref = pair(4, scb.grid_bins(B) if B in (1, 3, 256) else curriculum.grid({"serve_speed": (6.0, 9.0, B)}), scene.VARIANT_TT, SOA, seed=SEED, power=power, mix=mix)
    tot = totals(B, {b: (1 + b % 3, -5.0 + b) for b in range(0, B, 2)})
    for c in (h, ref):
        c.update(tot)
    assert np.array_equal(h.cdf, [((b + 1) << 24) // B for b in range(B)]) and np.array_equal(ref.cdf, h.cdf)
    assert np.array_equal(h.games, tot[0])                                                     # the statistics are still kept: the control run


def test_ranks_ties_unseen_bins_and_the_ema_bits():
    B = 6
    kw = dict(seed=SEED, power=1, mix=0.25, alpha=0.3)
    h, ref = pair(4, curriculum.grid({"serve_speed": (6.0, 9.0, B)}), scene.VARIANT_TT, SOA, **kw)
    # bins 0, 2 tie at -1; bin 1 scores 4; bin 3 scores -3 (the lowest); bins 4, 5 unseen
    tot = totals(B, {0: (2, -1.0), 1: (5, 4.0), 2: (1, -1.0), 3: (3, -3.0)})
    tot[2, 4] = 2                                                                              # two dropped games of an unseen bin
    for c in (h, ref):
        c.update(tot)
    assert not scb.same_words(h.words(), ref.words())
    assert np.array_equal(h.mean, np.array([-1, 4, -1, -3, 0, 0], F32)) and np.array_equal(h.games, [2, 5, 1, 3, 0, 0]) and np.array_equal(h.dropped, [0, 0, 0, 0, 2, 0])
    # ranks: 3 -> 1; 0 -> 2, 2 -> 3 (the tie breaks by index); 1 -> 4; unseen 4, 5 -> 1
    w = np.array([1 / 2, 1 / 4, 1 / 3, 1.0, 1.0, 1.0])
    p = 0.75 * w / w.sum() + 0.25 / B
    got = h.prob()
    assert np.allclose(got, p, atol=2.0 / ONE) and abs(got.sum() - 1.0) < 1e-12
    top = got.max() - 2.0 / ONE                                                               # (an interval's width is floored: one unit of 2^-24 either way)
    assert got[3] >= top and got[4] >= top and got[5] >= top and (got[:3] < top - 0.05).all()   # the lowest-mean seen bin and the unseen ones lead
    assert got[0] > got[2] > got[1]
    assert (np.diff(h.cdf.astype(I64)) >= 0).all() and h.cdf[-1] == ONE
    # a second horizon: the running mean moves by alpha, fp32, in the header's order; a first sighting takes the mean as it is
    tot2 = totals(B, {1: (4, -6.0), 4: (1, 2.5)})
    tot2[1, 1] += 3                                                                            # a sum that does not divide evenly
    for c in (h, ref):
        c.update(tot2)
    assert not scb.same_words(h.words(), ref.words())
    m = F32(np.float64(int(tot2[1, 1])) / (np.float64(65536.0) * np.float64(4)))
    assert h.mean[1] == F32(F32(4) + F32(F32(0.3) * F32(m - F32(4)))) and h.mean[4] == F32(2.5) and h.mean[0] == F32(-1)
    assert np.array_equal(h.games, [2, 9, 1, 3, 1, 0])
    got = h.prob()
    assert got[5] >= got.max() - 2.0 / ONE and got[3] >= got.max() - 2.0 / ONE                 # the one bin still unseen shares rank 1 with the lowest


def test_a_bin_with_an_empty_interval_is_never_drawn():
    B = 256
    h, ref = pair(64, scb.grid_bins(B), scene.VARIANT_TT, SOA, seed=SEED, power=4, mix=0.0)
    tot = totals(B, {b: (1, float(b)) for b in range(B)})                                       # bin b has rank b + 1
    for c in (h, ref):
        c.update(tot)
    assert not scb.same_words(h.words(), ref.words())
    width = np.diff(h.cdf.astype(I64), prepend=0)
    empty = np.nonzero(width == 0)[0]
    assert len(empty) > 50 and width[0] > ONE // 2 and h.cdf[-1] == ONE
    L = scb.lib()
    drawn = {L.curric_shim_bin(h.cdf.ctypes.data, B, L.curric_shim_u24(SEED, key, 0)) for key in range(20000)}
    drawn |= {L.curric_shim_bin(h.cdf.ctypes.data, B, int(u)) for u in np.concatenate([h.cdf[:-1].astype(I64), h.cdf[:-1].astype(I64) - 1, [0, ONE - 1]]).clip(0, ONE - 1)}
    assert not drawn & set(empty.tolist()) and 0 in drawn
    # ... and the envs the curriculum refills draw none of them either
    h.fill()
    h.cdf[:] = ref.cdf
    rew, reset = np.zeros(64, F32), np.ones(64, I64)
    fb, fq = np.zeros(64, np.int32), np.zeros(64, I64)
    for _ in range(20):
        h.step(rew, reset, fb, fq)
        assert not set(h.next_bin.tolist()) & set(empty.tolist())


def test_draw_frequencies_follow_the_table():
    L = scb.lib()
    p = np.array([0.4, 0.3, 0.2, 0.1])
    cdf = np.floor(np.cumsum(p) * ONE).astype(U32)
    cdf[-1] = ONE
    N = 4096
    bins = np.array([L.curric_shim_bin(cdf.ctypes.data, 4, L.curric_shim_u24(SEED, key, 0)) for key in range(N)])
    counts = np.bincount(bins, minlength=4)
    assert counts.sum() == N
    bound = 5.0 * np.sqrt(N * p * (1 - p))
    assert (np.abs(counts - N * p) <= bound).all(), (counts, N * p, bound)


# ------------------------------------------------------------------------------------------------------ 5. the library's refusals
FAKE = 0x1000          # a non-NULL "device pointer": every case below is refused before anything is dereferenced or copied


def _upload(L, **kw):
    bins = kw.pop("cells", [{"serve_speed": (6.0, 7.0)}, {"serve_speed": (7.0, 8.0)}])
    args = dict(num_envs=8, form=scene.VARIANT_TT, layout=SOA)
    args.update(kw)
    cur, arr, _ = scb.host_curric(args.pop("num_envs"), bins, args.pop("form"), args.pop("layout"), **args)
    rc = L.pp_serve_curric_upload(C.byref(cur), arr, FAKE, FAKE, None)
    return rc, L.ppenv_last_error().decode()


REFUSED = {
    "bins-0": (dict(n_bins=0), "bins outside 1 .. 256"),
    "bins-257": (dict(n_bins=257), "bins outside 1 .. 256"),
    "agents-3": (dict(num_agents=3), "num_agents not 1 or 2"),
    "power-neg": (dict(power=-1), "power outside 0 .. 4"),
    "power-5": (dict(power=5), "power outside 0 .. 4"),
    "mix-neg": (dict(mix=-0.01), "mix outside [0, 1] or alpha outside (0, 1], or one of them not finite"),
    "mix-above": (dict(mix=1.01), "mix outside [0, 1] or alpha outside (0, 1], or one of them not finite"),
    "mix-nan": (dict(mix=math.nan), "mix outside [0, 1] or alpha outside (0, 1], or one of them not finite"),
    "alpha-0": (dict(alpha=0.0), "mix outside [0, 1] or alpha outside (0, 1], or one of them not finite"),
    "alpha-above": (dict(alpha=1.5), "mix outside [0, 1] or alpha outside (0, 1], or one of them not finite"),
    "alpha-inf": (dict(alpha=math.inf), "mix outside [0, 1] or alpha outside (0, 1], or one of them not finite"),
    "envs-0": (dict(num_envs=0), "num_envs < 1"),
    "offset-neg": (dict(env_id_offset=-1), "env_id_offset < 0"),
    "form": (dict(form=99), "unknown form (a PPENV_VARIANT_* value)"),
    "layout": (dict(layout=2), "unknown layout"),
    "reset-rows": (dict(reset_rows=3), "reset_rows not 1 or 2"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_upload_refuses(case):
    kw, text = REFUSED[case]
    assert _upload(_lib.lib(), **dict(kw)) == (EINVAL, "pp_serve_curric_upload: " + text)


def test_upload_refuses_a_bad_cell_in_any_bin():
    L = _lib.lib()
    cur, arr, _ = scb.host_curric(8, scb.grid_bins(3), scene.VARIANT_TT, SOA)
    arr[2].speed_lo, arr[2].speed_hi = 9.0, 8.0                                                # the LAST bin: every bin is validated
    assert L.pp_serve_curric_upload(C.byref(cur), arr, FAKE, FAKE, None) == EINVAL
    assert L.ppenv_last_error().decode() == "pp_serve_curric_upload: a cell with a non-finite value or lo > hi"
    arr[2].speed_lo = 7.0
    arr[1].tilt_hi_deg = 57.5
    assert L.pp_serve_curric_upload(C.byref(cur), arr, FAKE, FAKE, None) == EINVAL
    assert L.ppenv_last_error().decode() == "pp_serve_curric_upload: a tilt or tilt_z bound beyond +-57 degrees (the short sine / cosine series)"
    arr[1].tilt_hi_deg = math.nan
    assert L.pp_serve_curric_upload(C.byref(cur), arr, FAKE, FAKE, None) == EINVAL
    for args in ((None, arr, FAKE, FAKE), (C.byref(cur), None, FAKE, FAKE), (C.byref(cur), arr, None, FAKE), (C.byref(cur), arr, FAKE, None)):
        assert L.pp_serve_curric_upload(*args, None) == EINVAL and L.ppenv_last_error().decode() == "pp_serve_curric_upload: NULL pointer"


def test_launches_refuse_null_and_sizes():
    L = _lib.lib()
    full = _lib.ServeCurricState(*([FAKE] * 8))
    holed = _lib.ServeCurricState(*([FAKE] * 7 + [None]))
    err = lambda: L.ppenv_last_error().decode()
    fill = "pp_serve_curric_fill: NULL pointer, num_envs <= 0 or bins outside 1 .. 256"
    for args in ((None, 4, 2, C.byref(full), FAKE), (FAKE, 4, 2, None, FAKE), (FAKE, 4, 2, C.byref(holed), FAKE), (FAKE, 4, 2, C.byref(full), None),
                 (FAKE, 0, 2, C.byref(full), FAKE), (FAKE, 4, 0, C.byref(full), FAKE), (FAKE, 4, 257, C.byref(full), FAKE)):
        assert L.pp_serve_curric_fill(*args, None) == EINVAL and err() == fill
    step = "pp_serve_curric_step: NULL pointer or num_envs <= 0"
    ok = [FAKE, 4, FAKE, FAKE, C.byref(full), FAKE, FAKE, FAKE]
    for k, bad in ((0, None), (1, 0), (2, None), (3, None), (4, None), (4, C.byref(holed)), (5, None), (6, None), (7, None)):
        args = list(ok)
        args[k] = bad
        assert L.pp_serve_curric_step(*args, None) == EINVAL and err() == step
    fold = "pp_serve_curric_fold: NULL pointer, count <= 0 or bins outside 1 .. 256"
    for args in ((None, FAKE, 8, 2, FAKE, FAKE), (FAKE, None, 8, 2, FAKE, FAKE), (FAKE, FAKE, 0, 2, FAKE, FAKE), (FAKE, FAKE, 8, 0, FAKE, FAKE),
                 (FAKE, FAKE, 8, 257, FAKE, FAKE), (FAKE, FAKE, 8, 2, None, FAKE), (FAKE, FAKE, scb.CHUNK + 1, 2, FAKE, None)):
        assert L.pp_serve_curric_fold(*args, None) == EINVAL and err() == fold
    update = "pp_serve_curric_update: NULL pointer or bins outside 1 .. 256"
    for args in ((None, 2, FAKE, C.byref(full)), (FAKE, 0, FAKE, C.byref(full)), (FAKE, 257, FAKE, C.byref(full)), (FAKE, 2, None, C.byref(full)),
                 (FAKE, 2, FAKE, None), (FAKE, 2, FAKE, C.byref(holed))):
        assert L.pp_serve_curric_update(*args, None) == EINVAL and err() == update
    assert L.pp_serve_curric_fold_bytes(0) == 0 and L.pp_serve_curric_fold_bytes(-5) == 0
    assert L.pp_serve_curric_fold_bytes(1) == L.pp_serve_curric_fold_bytes(scb.CHUNK) == 3 * 256 * 8
    assert L.pp_serve_curric_fold_bytes(scb.CHUNK + 1) == 2 * 3 * 256 * 8


# ------------------------------------------------------------------------------------------------------ 6. the grid and the CLI form
def test_grid_cuts_equal_intervals_last_axis_fastest():
    cells = curriculum.grid({"serve_speed": (6.0, 9.0, 4), "serve_tilt": (-5, 5, 3)})
    assert len(cells) == 12 and all(set(c) == {"serve_speed", "serve_tilt"} for c in cells)
    assert [c["serve_tilt"] for c in cells[:3]] == [(-5.0, -5.0 + 10.0 / 3), (-5.0 + 10.0 / 3, -5.0 + 20.0 / 3), (-5.0 + 20.0 / 3, 5.0)]
    assert all(c["serve_speed"] == (6.0, 6.75) for c in cells[:3]) and cells[3]["serve_speed"] == (6.75, 7.5) and cells[-1]["serve_speed"] == (8.25, 9.0)
    assert curriculum.ServeCurriculum.grid({"serve_speed": (6.0, 9.0, 4)}) == curriculum.grid({"serve_speed": (6.0, 9.0, 4)})
    assert curriculum.grid({}) == [{}]
    assert len(curriculum.grid({"serve_speed": (6, 9, 16), "serve_tilt": (-5, 5, 16)})) == 256
    with pytest.raises(ValueError, match="272 bins"):
        curriculum.grid({"serve_speed": (6, 9, 16), "serve_tilt": (-5, 5, 17)})
    for bad in ({"serve_speed": (6, 9)}, {"serve_speed": (6, 9, 0)}, {"serve_speed": (6, 9, 2.5)}, {"serve_speed": ("a", 9, 2)}):
        with pytest.raises(ValueError, match="not \\(lo, hi, bins\\)"):
            curriculum.grid(bad)
    with pytest.raises(ValueError, match="lo <= hi"):
        curriculum.grid({"serve_speed": (9, 6, 2)})
    with pytest.raises(ValueError, match="beyond \\+-57 degrees"):
        curriculum.grid({"serve_tilt": (-60, 5, 2)})


def test_grid_parse():
    assert curriculum.grid_parse(["serve_speed=6:9:4", "serve_tilt=-5:5:3"]) == {"serve_speed": (6.0, 9.0, 4), "serve_tilt": (-5.0, 5.0, 3)}
    assert curriculum.grid_parse([]) == {} and curriculum.grid_parse(None) == {}
    for bad in ("serve_speed", "serve_speed=6:9", "serve_speed=6:9:x", "serve_speed=6:9:4:1", "serve_speed=a:9:4"):
        with pytest.raises(ValueError, match="expected AXIS=LO:HI:BINS"):
            curriculum.grid_parse([bad])
