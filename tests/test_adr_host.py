"""Automatic domain randomisation (include/ppenv_dr_adr.h) without a GPU.  The rule is this project's own — no oracle pins it — so it is
checked against itself restated twice: the host build of the kernels' per-env and per-slot code (tests/csrc/adr_shim.cpp) against numpy
written from the header's words (adr_shim_binding.NumpyAdr), every word equal; with no boundary workers against the host build of the
reset-time plan (dr_shim_binding); then the update rule on hand-written totals, the draw's properties and frequencies, the refusals of the
real library's host-side validation, the ctypes mirrors, the CLI parser and scene.adr_draws."""
import ctypes as C
import math

import numpy as np
import pytest

import adr_shim_binding as ab
import dr_shim_binding as drb
from isaacgym_amd import _lib, adr, dr, scene

U32, F32, I32, I64 = np.uint32, np.float32, np.int32, np.int64
ONE = 1 << 24
EINVAL = -1
SEED = scene.stream_seed(42, scene.STREAM_TABLES)


def pair(n, dims, **kw):
    return ab.HostAdr(n, dims, **kw), ab.NumpyAdr(n, dims, **kw)


# ------------------------------------------------------------------------------------------------------ 1. the mirrors
def test_ctypes_mirrors_match_the_headers_layout():
    L = ab.lib()
    o = (C.c_size_t * 33)()
    L.adr_shim_layout(o)
    want = []
    for st in (_lib.AdrDim, _lib.Adr, _lib.AdrState):
        want += [C.sizeof(st)] + [getattr(st, name).offset for name, _ in st._fields_]
    assert list(o) == want and C.sizeof(_lib.AdrDim) == 32 and C.sizeof(_lib.Adr) == 48 + 8 * 32 and C.sizeof(_lib.AdrState) == 88
    k = (C.c_int64 * 5)()
    L.adr_shim_consts(k)
    assert list(k) == [_lib.ADR_COIN_INDEX, _lib.ADR_PICK_INDEX, _lib.ADR_MAX_SLOTS, scene.DR_MAX_TABLES, scene.DR_MAX_ROWS] == [512, 513, 17, 8, 64]
    assert _lib.ADR_COIN_INDEX == scene.DR_MAX_TABLES * scene.DR_MAX_ROWS                      # the first index no table row uses
    rng = np.random.default_rng(0)
    for sd, gid, j, k24 in zip(rng.integers(0, 2 ** 63, 200), rng.integers(0, 2 ** 32, 200), rng.integers(0, 2 ** 32, 200), rng.integers(0, 600, 200)):
        u = L.adr_shim_u24(int(sd), int(gid), int(j), int(k24))
        assert 0 <= u < ONE and F32(u) * F32(1.0 / 16777216.0) == F32(L.adr_shim_uniform(int(sd), int(gid), int(j), int(k24)))
    for frac, thr in ((0.0, 0), (1.0, ONE), (0.25, ONE // 4), (0.1, 1677721), (1e-9, 0)):
        assert L.adr_shim_thr(frac) == thr


# ------------------------------------------------------------------------------------------------------ 2. fill, step, fold, update together
@pytest.mark.parametrize("off", [0, 1000])
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("dims", list(ab.DIM_SETS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_host_build_equals_numpy_over_40_steps(n, dims, A, off):
    kw = dict(reset_rows=A, num_agents=A, seed=SEED, env_id_offset=off, **ab.SCRIPT_KW)
    h, ref = pair(n, ab.DIM_SETS[dims], **kw)
    assert not ab.same_words(h.words(), ref.words())
    assert (h.slot == -1).all() and (h.ret == 0).all() and (h.draws == 1).all()
    assert np.array_equal(h.range, [[F32(m["start"][0]), F32(m["start"][1])] for m in h.dims])
    rew, reset = ab.scripted(40, n, A, A)
    H = 8
    fs = [np.full((H, n), -1, I32) for _ in range(2)]
    fq = [np.zeros((H, n), I64) for _ in range(2)]
    first_game, staged = np.ones(n, bool), 0
    for t in range(40):
        r = t % H
        before, slot_before = h.words(), h.slot.copy()
        for k, c in enumerate((h, ref)):
            c.step(rew[t], reset[t], fs[k][r], fq[k][r])
        fired = reset[t][::A] != 0
        assert not ab.same_words(h.words(), ref.words()), (t, ab.same_words(h.words(), ref.words()))
        assert np.array_equal(fs[0][r], fs[1][r]) and np.array_equal(fq[0][r][fired], fq[1][r][fired]), t
        after = h.words()
        for name in after:                                                        # nothing of a non-resetting env changes, bit for bit
            if name.startswith("table"):
                assert np.array_equal(before[name][:, ~fired], after[name][:, ~fired]), (t, name)
        for name in ("draws", "slot"):
            assert np.array_equal(before[name][~fired], after[name][~fired]), (t, name)
        assert np.array_equal(after["draws"][fired], before["draws"][fired] + 1)
        assert (fs[0][r][~fired] == -1).all() and np.array_equal(fs[0][r][fired], slot_before[fired])
        assert (fs[0][r][fired & first_game] == -1).all() and (fs[0][r][fired & ~first_game] >= 0).all()
        assert (h.ret[fired] == 0).all() and (h.slot[fired] >= 0).all() and (h.slot[fired] <= 2 * h.D).all()
        staged += int((fs[0][r] >= 0).sum())
        first_game &= ~fired
        if r == H - 1:
            tots = [c.fold(fs[k], fq[k]) for k, c in enumerate((h, ref))]
            assert np.array_equal(tots[0], tots[1])
            for c, tot in zip((h, ref), tots):
                c.update(tot)
            assert not ab.same_words(h.words(), ref.words()), (t, "update", ab.same_words(h.words(), ref.words()))
            for d, m in enumerate(h.dims):
                assert F32(m["limit"][0]) <= h.range[d, 0] <= F32(m["start"][0]) <= F32(m["start"][1]) <= h.range[d, 1] <= F32(m["limit"][1])
    assert int(h.games.sum() + h.dropped.sum()) == staged
    if n >= 63:
        assert int(h.dropped.sum()) >= 1                                          # inf, nan and beyond 2^31: counted apart, never in a mean
    if n in (63, 64, 65) and dims != "one":                                       # ten boundaries of a few games each: the script moves some each way
        assert int(h.widened.sum()) >= 1 and int(h.narrowed.sum()) >= 1
    assert np.isfinite(h.mean).all()


# ------------------------------------------------------------------------------------------------------ 3. no boundary workers: the reset-time plan's bits
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("dims", ["rows7", "rows27"])
def test_boundary_frac_0_writes_what_the_reset_time_plan_writes(dims, A):
    n, D = 65, ab.DIM_SETS[dims]
    names = dr.TABLE_NAMES
    plan = {"frequency": 1, "tables": {name: dict(rows=m["rows"], distribution="uniform", operation="scaling", range=m["start"], schedule=None, schedule_steps=0)
                                       for name, m in zip(names, D)}}
    host_dr = drb.HostDR(plan, n, seed=SEED, env_id_offset=7, reset_rows=A)
    h = ab.HostAdr(n, D, reset_rows=A, num_agents=A, seed=SEED, env_id_offset=7, boundary_frac=0.0, min_games=1, t_low=-ab.FLT_MAX, t_high=ab.FLT_MAX)
    host_dr.apply(np.zeros(A * n, I64))                                           # the first application redraws every env: the fill
    same = lambda: all(np.array_equal(host_dr.tables[name].view(U32), t.view(U32)) for name, t in zip(names, h.tables))
    assert same() and np.array_equal(host_dr.draws, h.draws)
    rew, reset = ab.scripted(40, n, A, A)
    fs, fq = np.zeros(n, I32), np.zeros(n, I64)
    for t in range(40):
        host_dr.apply(reset[t])
        h.step(rew[t], reset[t], fs, fq)
        assert same() and np.array_equal(host_dr.draws, h.draws), t
        assert (h.slot[h.draws > 1] == 2 * len(D)).all()
    assert any(np.unique(t).size > 2 for t in h.tables)


# ------------------------------------------------------------------------------------------------------ 4. the update rule
def totals(S, games):
    """tot for {slot: (n, mean return)}; a mean that is a multiple of 2^-16 is exact"""
    tot = np.zeros((3, S), I64)
    for s, (n, mean) in games.items():
        tot[0, s], tot[1, s] = n, int(round(mean * 65536.0)) * n
    return tot


def both(dims, **kw):
    return pair(4, dims, seed=SEED, **kw)


def test_update_thresholds_are_inclusive_and_in_between_only_clears():
    dims = [ab.dim(7, (1.0, 1.0), (0.5, 2.0), 0.125), ab.dim(1, (0.75, 1.25), (0.5, 2.0), 0.25)]
    for c in both(dims, min_games=4, t_low=-2.0, t_high=3.0):
        # slot 0 (dim 0 lo): exactly t_high widens; slot 1 (dim 0 hi): exactly t_low "narrows" (clamped at the start); slot 3: in between
        c.update(totals(5, {0: (4, 3.0), 1: (4, -2.0), 3: (5, 0.5), 4: (9, -7.0)}))
        assert np.array_equal(c.range, np.array([[0.875, 1.0], [0.75, 1.25]], F32))
        assert c.widened.tolist() == [1, 0, 0, 0, 0] and c.narrowed.tolist() == [0, 1, 0, 0, 0]
        assert np.array_equal(c.mean, np.array([3.0, -2.0, 0.0, 0.5, -7.0], F32))
        assert not c.acc_n.any() and not c.acc_q.any() and c.games.tolist() == [4, 4, 0, 5, 9]    # judged slots clear, the interior keeps its mean only
        # just below t_high / just above t_low: cleared, not moved
        c.update(totals(5, {0: (4, 3.0 - 2.0 ** -16), 1: (4, -2.0 + 2.0 ** -16)}))
        assert np.array_equal(c.range, np.array([[0.875, 1.0], [0.75, 1.25]], F32)) and c.widened.sum() == 1 and c.narrowed.sum() == 1
        assert not c.acc_n.any() and c.mean[0] == F32(3.0 - 2.0 ** -16)


def test_update_carries_a_slot_below_min_games_over():
    dims = [ab.dim(7, (1.0, 1.0), (0.5, 2.0), 0.125)]
    for c in both(dims, min_games=10, t_low=-1.0, t_high=1.0):
        c.update(totals(3, {1: (6, 5.0)}))
        assert c.acc_n.tolist() == [0, 6, 0] and c.acc_q[1] == 6 * 5 * 65536 and c.mean[1] == 0 and c.range[0, 1] == 1.0 and c.games[1] == 6
        c.update(totals(3, {1: (4, -5.0)}))                                       # 10 games now: the mean is over both updates' games
        assert c.acc_n.tolist() == [0, 0, 0] and c.mean[1] == F32(1.0) and c.range[0, 1] == F32(1.125) and c.widened[1] == 1 and c.games[1] == 10


def test_update_clamps_at_limit_and_at_start_and_moves_both_sides_at_once():
    dims = [ab.dim(7, (0.9, 1.1), (0.8, 1.25), 0.07)]
    for c in both(dims, min_games=1, t_low=-1.0, t_high=1.0):
        c.update(totals(3, {0: (1, 2.0), 1: (1, 2.0)}))                           # both sides of one dim in one update
        assert np.array_equal(c.range, np.array([[F32(F32(0.9) - F32(0.07)), F32(F32(1.1) + F32(0.07))]], F32))
        c.update(totals(3, {0: (1, 2.0), 1: (1, 2.0)}))
        assert np.array_equal(c.range, np.array([[0.8, F32(F32(F32(1.1) + F32(0.07)) + F32(0.07))]], F32))   # lo clamped at its limit
        c.update(totals(3, {0: (1, 2.0), 1: (1, 2.0)}))
        assert np.array_equal(c.range, np.array([[0.8, 1.25]], F32)) and c.widened.tolist() == [3, 3, 0]
        for _ in range(5):
            c.update(totals(3, {0: (1, -2.0), 1: (1, -2.0)}))
        assert np.array_equal(c.range, np.array([[0.9, 1.1]], F32)) and c.narrowed.tolist() == [5, 5, 0]    # clamped at the starts


def test_update_counts_dropped_games_and_never_averages_them():
    dims = [ab.dim(7, (1.0, 1.0), (0.5, 2.0), 0.125)]
    for c in both(dims, min_games=2, t_low=-1.0, t_high=1.0):
        tot = totals(3, {0: (1, 9.0)})
        tot[2] = [5, 0, 2]
        c.update(tot)
        assert c.dropped.tolist() == [5, 0, 2] and c.games.tolist() == [1, 0, 0] and c.acc_n.tolist() == [1, 0, 0] and c.range[0, 0] == 1.0
        c.update(tot)
        assert c.dropped.tolist() == [10, 0, 4] and c.mean[0] == 9.0 and c.range[0, 0] == F32(0.875)


def test_update_keeps_the_invariant_over_200_random_updates():
    rng = np.random.default_rng(5)
    h, ref = both(ab.DIMS_7, min_games=3, t_low=-0.5, t_high=0.5)
    for k in range(200):
        tot = np.zeros((3, 11), I64)
        tot[0] = rng.integers(0, 6, 11)
        tot[1] = (rng.normal(0.0, 1.0, 11) * 65536.0).astype(I64) * tot[0]
        tot[2] = rng.integers(0, 2, 11)
        for c in (h, ref):
            c.update(tot)
        assert not ab.same_words(h.words(), ref.words()), k
        for d, m in enumerate(ab.DIMS_7):
            assert F32(m["limit"][0]) <= h.range[d, 0] <= F32(m["start"][0]) <= F32(m["start"][1]) <= h.range[d, 1] <= F32(m["limit"][1]), (k, d)
    assert h.widened.sum() > 20 and h.narrowed.sum() > 20


# ------------------------------------------------------------------------------------------------------ 5. the draw
def test_a_boundary_worker_holds_the_boundarys_own_bits():
    dims = [ab.dim(7, (0.7, 1.3), (0.5, 1.5), 0.1), ab.dim(7, (0.9, 1.2), (0.5, 1.5), 0.1), ab.dim(1, (0.6, 1.1), (0.5, 1.5), 0.1)]
    n = 512
    h = ab.HostAdr(n, dims, seed=SEED, boundary_frac=0.5, min_games=1, t_low=-ab.FLT_MAX, t_high=ab.FLT_MAX)
    fs, fq = np.zeros(n, I32), np.zeros(n, I64)
    h.step(np.zeros(n, F32), np.ones(n, I64), fs, fq)
    assert set(h.slot.tolist()) == set(range(7))
    for d, t in enumerate(h.tables):
        lo, hi = h.range[d]
        assert ((t >= lo) & (t <= hi)).all()
        for side, v in ((0, lo), (1, hi)):
            pinned = h.slot == 2 * d + side
            assert pinned.any() and (t[:, pinned].view(U32) == v.view(U32)).all()
        free = h.slot >> 1 != d
        assert np.unique(t[:, free]).size > free.sum() // 2                                   # the others are drawn inside [lo, hi]


def test_boundary_share_and_slot_frequencies():
    """N = 4096 envs, 8 draws each, boundary_frac 0.5, D = 3: the share within 5 binomial sigma of thr / 2^24, each of the 6 slots within 5 of
    its sixth.  (The seed was checked under NumpyAdr's np_slots alone before this was written.)"""
    N, J, D = 4096, 8, 3
    thr = ONE // 2
    gid, j = np.meshgrid(np.arange(N), np.arange(J), indexing="ij")
    slots = ab.np_slots(SEED, gid.ravel(), j.ravel(), thr, D)
    L = ab.lib()
    assert all(L.adr_shim_slot(SEED, int(g), int(k), thr, D) == int(s) for g, k, s in zip(gid.ravel()[::37], j.ravel()[::37], slots[::37]))
    M = N * J
    workers = int((slots < 2 * D).sum())
    p = thr / ONE
    assert abs(workers - M * p) <= 5.0 * math.sqrt(M * p * (1 - p)), (workers, M * p)
    counts = np.bincount(slots[slots < 2 * D], minlength=2 * D)
    assert (np.abs(counts - workers / 6.0) <= 5.0 * math.sqrt(workers * (1 / 6) * (5 / 6))).all(), counts


# ------------------------------------------------------------------------------------------------------ 6. the library's refusals
FAKE = 0x1000          # a non-NULL "device pointer": every case below is refused before anything is dereferenced or copied


def _upload(L, frac=0.25, dim_over=None, **kw):
    dims = [dict(ab.DIMS_1[0]), dict(ab.DIMS_7[4])]
    ptrs = [FAKE, FAKE]
    if dim_over:
        for k, v in dim_over.items():
            if k == "table":
                ptrs[1] = v
            else:
                dims[1][k] = v
    args = dict(num_envs=8, boundary_frac=0.25)
    args.update(kw)
    A = ab.host_adr(args.pop("num_envs"), dims, ptrs, **args)
    rc = L.pp_dr_adr_upload(C.byref(A), frac, FAKE, None)
    return rc, L.ppenv_last_error().decode()


REFUSED = {
    "envs-0": (dict(num_envs=0), "num_envs < 1"),
    "offset-neg": (dict(env_id_offset=-1), "env_id_offset < 0"),
    "reset-rows": (dict(reset_rows=3), "reset_rows not 1 or 2"),
    "agents-0": (dict(num_agents=0), "num_agents not 1 or 2"),
    "dims-0": (dict(n_dims=0), "dims outside 1 .. 8"),
    "dims-9": (dict(n_dims=9), "dims outside 1 .. 8"),
    "frac-neg": (dict(frac=-0.01), "boundary_frac outside [0, 1] or not finite"),
    "frac-above": (dict(frac=1.01), "boundary_frac outside [0, 1] or not finite"),
    "frac-nan": (dict(frac=math.nan), "boundary_frac outside [0, 1] or not finite"),
    "games-0": (dict(min_games=0), "min_games < 1"),
    "low-above-high": (dict(t_low=1.0, t_high=0.5), "t_low or t_high not finite, or t_low > t_high"),
    "high-inf": (dict(t_high=math.inf), "t_low or t_high not finite, or t_low > t_high"),
    "low-nan": (dict(t_low=math.nan), "t_low or t_high not finite, or t_low > t_high"),
    "table-null": (dict(dim_over=dict(table=None)), "dim 1: a NULL table"),
    "rows-0": (dict(dim_over=dict(rows=0)), "dim 1: rows outside 1 .. 64"),
    "rows-65": (dict(dim_over=dict(rows=65)), "dim 1: rows outside 1 .. 64"),
    "start-nan": (dict(dim_over=dict(start=(math.nan, 1.0))), "dim 1: a non-finite start_lo, start_hi, limit_lo, limit_hi or step"),
    "limit-inf": (dict(dim_over=dict(limit=(0.5, math.inf))), "dim 1: a non-finite start_lo, start_hi, limit_lo, limit_hi or step"),
    "step-0": (dict(dim_over=dict(step=0.0)), "dim 1: step <= 0"),
    "step-neg": (dict(dim_over=dict(step=-0.1)), "dim 1: step <= 0"),
    "limit-lo-0": (dict(dim_over=dict(limit=(0.0, 1.6))), "dim 1: limit_lo <= 0"),
    "start-below-limit": (dict(dim_over=dict(start=(0.3, 1.3))), "dim 1: not limit_lo <= start_lo <= start_hi <= limit_hi"),
    "start-crossed": (dict(dim_over=dict(start=(1.3, 0.7))), "dim 1: not limit_lo <= start_lo <= start_hi <= limit_hi"),
    "start-above-limit": (dict(dim_over=dict(start=(0.7, 1.7))), "dim 1: not limit_lo <= start_lo <= start_hi <= limit_hi"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_upload_refuses(case):
    kw, text = REFUSED[case]
    assert _upload(_lib.lib(), **dict(kw)) == (EINVAL, "pp_dr_adr_upload: " + text)


def test_launches_refuse_null_and_sizes():
    L = _lib.lib()
    full = _lib.AdrState(*([FAKE] * 11))
    holed = _lib.AdrState(*([FAKE] * 10 + [None]))
    err = lambda: L.ppenv_last_error().decode()
    A = ab.host_adr(8, ab.DIMS_1, [FAKE])
    for args in ((None, 0.25, FAKE), (C.byref(A), 0.25, None)):
        assert L.pp_dr_adr_upload(*args, None) == EINVAL and err() == "pp_dr_adr_upload: NULL pointer"
    fill = "pp_dr_adr_fill: NULL pointer, num_envs <= 0 or dims outside 1 .. 8"
    for args in ((None, 4, 2, C.byref(full)), (FAKE, 4, 2, None), (FAKE, 4, 2, C.byref(holed)), (FAKE, 0, 2, C.byref(full)), (FAKE, 4, 0, C.byref(full)),
                 (FAKE, 4, 9, C.byref(full))):
        assert L.pp_dr_adr_fill(*args, None) == EINVAL and err() == fill
    step = "pp_dr_adr_step: NULL pointer or num_envs <= 0"
    ok = [FAKE, 4, FAKE, FAKE, C.byref(full), FAKE, FAKE]
    for k, bad in ((0, None), (1, 0), (2, None), (3, None), (4, None), (4, C.byref(holed)), (5, None), (6, None)):
        args = list(ok)
        args[k] = bad
        assert L.pp_dr_adr_step(*args, None) == EINVAL and err() == step
    update = "pp_dr_adr_update: NULL pointer or dims outside 1 .. 8"
    for args in ((None, 2, FAKE, C.byref(full)), (FAKE, 0, FAKE, C.byref(full)), (FAKE, 9, FAKE, C.byref(full)), (FAKE, 2, None, C.byref(full)),
                 (FAKE, 2, FAKE, None), (FAKE, 2, FAKE, C.byref(holed))):
        assert L.pp_dr_adr_update(*args, None) == EINVAL and err() == update


# ------------------------------------------------------------------------------------------------------ 7. the Python surface
def test_parse():
    assert adr.parse(["link_mass_scale=1:1:0.6:1.4:0.05", "friction_scale=0.9:1.1:0.4:1.6:0.1"]) == {
        "link_mass_scale": dict(start=(1.0, 1.0), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(0.9, 1.1), limit=(0.4, 1.6), step=0.1)}
    assert adr.parse([]) == {} and adr.parse(None) == {}
    for bad in ("link_mass_scale", "link_mass_scale=1:1:0.6:1.4", "link_mass_scale=1:1:0.6:1.4:x", "link_mass_scale=1:1:0.6:1.4:0.05:2"):
        with pytest.raises(ValueError, match="expected TABLE=START_LO:START_HI:LIMIT_LO:LIMIT_HI:STEP"):
            adr.parse([bad])


def test_check_parameters_names_the_argument():
    assert adr.check_parameters(0.25, 256, -1.0, 2) == (0.25, 256, -1.0, 2.0)
    assert adr.check_parameters(0, 1, 0.0, 0.0) == (0.0, 1, 0.0, 0.0)
    for args, name in (((-0.1, 1, 0, 1), "boundary_frac"), ((1.5, 1, 0, 1), "boundary_frac"), ((math.nan, 1, 0, 1), "boundary_frac"), (("x", 1, 0, 1), "boundary_frac"),
                       ((0.5, 0, 0, 1), "min_games"), ((0.5, 2.5, 0, 1), "min_games"), ((0.5, True, 0, 1), "min_games"),
                       ((0.5, 1, math.inf, 1), "t_low"), ((0.5, 1, 0, math.nan), "t_high"), ((0.5, 1, 0, 1e39), "t_high"), ((0.5, 1, 2, 1), "t_low")):
        with pytest.raises(ValueError, match=name):
            adr.check_parameters(*args)


def test_check_dims_orders_validates_and_names_the_field():
    good = {"friction_scale": dict(start=(1, 1), limit=(0.4, 1.6), step=0.1), "link_mass_scale": dict(start=[0.9, 1.1], limit=[0.6, 1.4], step=0.05)}
    out = adr.check_dims(good)
    assert list(out) == ["link_mass_scale", "friction_scale"]                                  # dr.TABLE_NAMES' order, whatever the dict's
    assert out["friction_scale"] == dict(start=(1.0, 1.0), limit=(0.4, 1.6), step=0.1)
    rows7 = {"dof_stiffness_scale": 7, "link_mass_scale": 7}
    with pytest.raises(ValueError, match="no table 'friction_scale'"):
        adr.check_dims(good, rows7)
    for bad, text in (({}, "at least one table"), ({"mass": good["friction_scale"]}, "no table 'mass'"),
                      ({"friction_scale": dict(start=(1, 1), limit=(0.4, 1.6))}, "expected dict"),
                      ({"friction_scale": dict(start=(1, 1, 1), limit=(0.4, 1.6), step=0.1)}, "expected dict"),
                      ({"friction_scale": dict(start=(1, math.inf), limit=(0.4, 1.6), step=0.1)}, "start hi inf is not finite"),
                      ({"friction_scale": dict(start=(1, 1), limit=(0.4, 1.6), step=0)}, "step 0.0 must be above 0"),
                      ({"friction_scale": dict(start=(1, 1), limit=(0, 1.6), step=0.1)}, "limit lo 0.0 must be above 0"),
                      ({"friction_scale": dict(start=(0.3, 1), limit=(0.4, 1.6), step=0.1)}, "not limit lo <= start lo"),
                      ({"friction_scale": dict(start=(1.2, 1), limit=(0.4, 1.6), step=0.1)}, "not limit lo <= start lo"),
                      ({"friction_scale": dict(start=(1, 1.7), limit=(0.4, 1.6), step=0.1)}, "not limit lo <= start lo")):
        with pytest.raises(ValueError, match=text):
            adr.check_dims(bad)


def test_table_json_and_lines():
    class Stub:                                                                                # what table_json reads of an AutoRandomizer
        dims = adr.check_dims({"link_mass_scale": dict(start=(1, 1), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(0.9, 1.1), limit=(0.4, 1.6), step=0.1)})
        names, D, boundary_frac, min_games, t_low, t_high = list(dims), 2, 0.25, 256, -2.0, 3.0

        def table(self):
            return dict(lo=np.array([0.85, 0.9], F32), hi=np.array([1.0, 1.3], F32), games=np.array([10, 20, 30, 40, 500], I64), mean=np.array([3.5, 1, -2.5, 0, 1.25], F32),
                        dropped=np.array([0, 0, 1, 0, 2], I64), widened=np.array([3, 0, 0, 2, 0], I32), narrowed=np.array([0, 0, 1, 0, 0], I32))
    t = adr.table_json(Stub(), epoch=7)
    assert t["epoch"] == 7 and [d["table"] for d in t["dims"]] == ["link_mass_scale", "friction_scale"] and t["interior"] == dict(games=500, mean_return=1.25, dropped=2)
    assert t["dims"][0]["lo"] == float(F32(0.85)) and t["dims"][0]["lo_side"] == dict(games=10, mean_return=3.5, dropped=0, widened=3, narrowed=0)
    assert t["dims"][1]["hi_side"]["widened"] == 2 and t["dims"][1]["lo_side"]["dropped"] == 1
    lines = adr.table_lines(t)
    assert len(lines) == 4 and lines[0] == "adr at epoch 7: 2 dims, boundary share 0.25, widen at 3, narrow at -2, judged every 256 games"
    assert lines[1].startswith("  link_mass_scale: [0.85, 1]  (start 1..1, limit 0.6..1.4)  lo: games 10 mean 3.5 +3 -0  hi: games 20 mean 1 +0 -0")
    assert "dropped 1" in lines[2] and lines[3] == "  interior: games 500 mean 1.25 dropped 2"
    import json
    json.dumps(t)


@pytest.mark.parametrize("dims", list(ab.DIM_SETS))
def test_scene_adr_draws_predicts_numpy_adr(dims):
    n, D = 65, ab.DIM_SETS[dims]
    ref = ab.NumpyAdr(n, D, seed=SEED, env_id_offset=1000, **ab.SCRIPT_KW)
    rew, reset = ab.scripted(24, n, 1, 1)
    ab.run(ref, rew, reset, 8)                                                   # ranges that have moved, envs at different draw counts
    fs, fq = np.zeros(n, I32), np.zeros(n, I64)
    draws = ref.draws.copy()
    ref.step(np.zeros(n, F32), np.ones(n, I64), fs, fq)
    slots, cols = scene.adr_draws(SEED, 1000 + np.arange(n), draws, [m["rows"] for m in D], ref.range, ref.thr)
    assert np.array_equal(slots, ref.slot) and slots.dtype == I32
    for d, c in enumerate(cols):
        assert np.array_equal(c.view(U32), ref.tables[d].view(U32)), d
    with pytest.raises(ValueError, match="adr_draws"):
        scene.adr_draws(SEED, [0], [0], [65], [[1, 1]], 0)
