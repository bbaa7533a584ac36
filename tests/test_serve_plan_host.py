"""The serve plan (include/ppenv_serve.h) without a GPU: the host build of the kernels' per-env code (tests/csrc/serve_shim.cpp) against a
numpy restatement of the draw, the rule of the per-step launch, the refusals of the upload / Sweep / CLI, and the keying of its stream."""
import ctypes as C

import numpy as np
import pytest

import serve_shim_binding as ssb
from isaacgym_amd import _lib, policy, scene, serve, vec_task

U32, U64, F32 = np.uint32, np.uint64, np.float32
SOA, AOS = _lib.SERVE_LAYOUT_SOA3, _lib.SERVE_LAYOUT_AOS5
FORMS = {"T3": scene.VARIANT_T3, "TT": scene.VARIANT_TT, "TN": scene.VARIANT_TN, "T4": scene.VARIANT_T4}
NOISE_SALT = 0x5DEECE66D
EINVAL = -1


# ---- numpy restatement of ppenv_device.h's counter RNG (as tests/test_rng_streams_host.py restates it) and of the serve draw, in fp32
def hash32(x):
    x = np.atleast_1d(np.asarray(x, U32))
    x = (x ^ (x >> U32(16))) * U32(0x7FEB352D)
    x = (x ^ (x >> U32(15))) * U32(0x846CA68B)
    return x ^ (x >> U32(16))


def ubits(kseed, gid, episode, k):
    """rng_uniform's 24-bit integer (the float is this x 2^-24), broadcast over arrays of gid / episode / k."""
    ks, gid, episode, k = np.atleast_1d(np.asarray(kseed, U64)), np.atleast_1d(np.asarray(gid, U32)), np.atleast_1d(np.asarray(episode, U32)), np.atleast_1d(np.asarray(k, U32))
    lo, hi = (ks & U64(0xFFFFFFFF)).astype(U32), (ks >> U64(32)).astype(U32)
    h = hash32(gid ^ lo)
    h = hash32(h + episode * U32(0x9E3779B9) + hi)
    h = hash32(h + (k + U32(1)) * U32(0x85EBCA6B))
    return h >> U32(8)


def rows_of(a):
    a = np.ascontiguousarray(a)
    return set(a.view(np.dtype((np.void, a.dtype.itemsize * a.shape[1]))).ravel().tolist())


def shared(a, b):
    """number of rows of `a` that are a row of `b`; the rows of each must be distinct among themselves"""
    sa, sb_ = rows_of(a), rows_of(b)
    assert len(sa) == len(a) and len(sb_) == len(b), "streams of one seed collide"
    return len(sa & sb_)


def sincos_small(x):
    one = F32(1)
    x2 = x * x
    s = x * (one + x2 * (F32(-1) / F32(6) + x2 * (one / F32(120) + x2 * (F32(-1) / F32(5040) + x2 * (one / F32(362880))))))
    c = one + x2 * (F32(-0.5) + x2 * (one / F32(24) + x2 * (F32(-1) / F32(720) + x2 * (one / F32(40320)))))
    return s, c


def np_serve(resolved, n, form, layout, seed, env_id_offset, paired, count):
    """serve(e, count[e]) for every env -> the `out` buffer of that layout, every operation rounded to fp32 on its own."""
    G = len(resolved)
    S = n // G
    e = np.arange(n)
    key = (e % S if paired else env_id_offset + e).astype(U32)
    cell = lambda axis, side: np.array([resolved[g][axis][side] for g in e // S], F32)

    def quantity(axis, k):
        u = ubits(seed, key, count.astype(U32), k).astype(F32) * F32(1.0 / 16777216.0)
        lo, hi = cell(axis, 0), cell(axis, 1)
        return lo + (hi - lo) * u
    speed, tilt = quantity("serve_speed", 0), quantity("serve_tilt", 1)
    tilt_z = np.zeros(n, F32) if form == scene.VARIANT_T3 else quantity("serve_tilt_z", 2)
    deg = F32(0.017453292519943295)
    sa, ca = sincos_small(tilt * deg)
    sz, cz = sincos_small(tilt_z * deg)
    if form == scene.VARIANT_T3:
        v = (-speed * ca, -speed * sa, np.zeros(n, F32))
    elif form in (scene.VARIANT_TT, scene.VARIANT_T4):
        v = (-speed * ca * cz, -speed * sa * sz, -speed * sa)
    else:
        v = (-speed * ca * cz, speed * sa * cz, speed * sz)
    if layout == SOA:
        return np.stack(v).astype(F32)
    return np.stack([quantity("ball_y", 3), quantity("ball_z", 4)] + list(v), axis=1).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def env_column(out, layout, mask):
    """the part of `out` that belongs to the envs of `mask`, as bits"""
    return bits(out)[:, mask] if layout == SOA else bits(out)[mask]


# ------------------------------------------------------------------------------------------------------ 1. shim = numpy, bitwise
@pytest.mark.parametrize("paired", [False, True], ids=["global-key", "paired"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("layout", [SOA, AOS], ids=["soa3", "aos5"])
@pytest.mark.parametrize("form", list(FORMS))
def test_shim_is_the_numpy_restatement(form, layout, G, paired):
    n, seed, off = 21, scene.stream_seed(42, scene.STREAM_SERVES), 5
    cells = [{"serve_speed": (6.0 + g, 6.5 + g), "serve_tilt": (-7.0, 3.0 + g), "serve_tilt_z": (-2.0, 9.0), "ball_y": (-0.3, 0.1 * g), "ball_z": (0.9, 1.0)} for g in range(G)]
    h = ssb.HostServe(n, cells, FORMS[form], layout, seed=seed, env_id_offset=off, paired=paired)
    resolved = serve.resolve_cells(cells, ssb.DEFAULTS, serve.AXES_27DOF)
    count = np.zeros(n, np.uint32)
    want = np_serve(resolved, n, FORMS[form], layout, seed, off, paired, count)
    assert np.array_equal(bits(h.out), bits(want)) and np.array_equal(h.count, count)
    assert len(np.unique(bits(want))) > n                                        # (not a buffer of zeros)
    for r in ssb.scripted_resets(16, n, 1):
        h.apply(r)
        fired = r != 0
        count = count + fired.astype(np.uint32)
        new = np_serve(resolved, n, FORMS[form], layout, seed, off, paired, count)
        if layout == SOA:
            want[:, fired] = new[:, fired]
        else:
            want[fired] = new[fired]
        assert np.array_equal(h.count, count)
        assert np.array_equal(bits(h.out), bits(want))
    assert count.max() >= 4 and count.min() >= 0
    # the velocity is serve_from_draws of THIS unit: spot values against fp64
    v = ssb.velocity(scene.VARIANT_TN, 5.5, -4.0, 12.0)
    a, az = np.deg2rad(-4.0), np.deg2rad(12.0)
    np.testing.assert_allclose(v, [-5.5 * np.cos(a) * np.cos(az), 5.5 * np.sin(a) * np.cos(az), 5.5 * np.sin(az)], rtol=2e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------------ 2. the rule
@pytest.mark.parametrize("reset_rows", [1, 2])
@pytest.mark.parametrize("layout", [SOA, AOS], ids=["soa3", "aos5"])
def test_rule_only_flagged_envs_advance(reset_rows, layout):
    n = 37
    h = ssb.HostServe(n, ssb.two_cells()[:1], scene.VARIANT_TT, layout, reset_rows=reset_rows, seed=9)
    seq = ssb.scripted_resets(24, n, reset_rows)
    assert (seq == 2 ** 32).any() and (seq == 1).any()
    if reset_rows == 2:
        seq[3, 2 * 4 + 1] = 1                                                    # row 2 e + 1 alone is NOT read: env 4 does not advance for it
        assert seq[3, 2 * 4] == 0
    count = np.zeros(n, np.uint32)
    for t, r in enumerate(seq):
        before_out, before_count = h.out.copy(), h.count.copy()
        if t == 12:                                                              # an id call in the middle: listed envs advance, out-of-range ids are skipped
            ids = np.array([3, n - 1, -1, n, 2 ** 40, 0, 3], np.int64)
            h.apply_ids(ids)
            fired = np.zeros(n, bool)
            fired[[0, 3, n - 1]] = True
        else:
            h.apply(r)
            fired = r[::reset_rows] != 0
        count = count + fired.astype(np.uint32)
        assert np.array_equal(h.count, count), t
        assert np.array_equal(env_column(h.out, layout, ~fired), env_column(before_out, layout, ~fired)), t       # untouched, bit for bit
        assert not np.array_equal(env_column(h.out, layout, fired), env_column(before_out, layout, fired)) or not fired.any()
        assert np.array_equal(h.count[~fired], before_count[~fired])
    # the buffer always holds serve(e, count[e]): a fresh fill at these counts reproduces it
    again = ssb.HostServe(n, ssb.two_cells()[:1], scene.VARIANT_TT, layout, reset_rows=reset_rows, seed=9)
    again.count[:] = count
    again.fill()
    assert np.array_equal(bits(again.out), bits(h.out))


# ------------------------------------------------------------------------------------------------------ 3. a pinned cell
@pytest.mark.parametrize("form", list(FORMS))
def test_pinned_cell_gives_exactly_the_pinned_value(form):
    n = 16
    pin = {"serve_speed": 7.25, "serve_tilt": -3.5, "serve_tilt_z": 0.0 if form == "T3" else 6.0, "ball_y": -0.125, "ball_z": 1.0}
    h = ssb.HostServe(n, [pin], FORMS[form], AOS, seed=3)
    v = ssb.velocity(FORMS[form], 7.25, -3.5, pin["serve_tilt_z"])
    want = np.concatenate([np.array([-0.125, 1.0], F32), v])
    for _ in range(5):
        assert np.array_equal(bits(h.out), np.tile(bits(want), (n, 1)))
        h.apply(np.ones(n, np.int64))
    assert h.count.tolist() == [5] * n
    zero = ssb.HostServe(n, [{"serve_speed": 7.0, "serve_tilt": 0.0, "serve_tilt_z": 0.0}], FORMS[form], SOA, seed=3)
    assert np.array_equal(bits(zero.out), np.tile(bits(ssb.velocity(FORMS[form], 7.0, 0.0, 0.0))[:, None], (1, n)))


# ------------------------------------------------------------------------------------------------------ 4. refusals
BAD_PLANS = {"tilt beyond 57": dict(cells=[{"serve_tilt": (-5.0, 57.5)}]), "tilt_z beyond -57": dict(cells=[{"serve_tilt_z": (-58.0, 0.0)}]),
             "lo > hi": dict(raw=("speed_lo", 9.0)), "nan": dict(raw=("ball_y_hi", float("nan"))), "inf": dict(raw=("speed_hi", float("inf"))),
             "groups * S != N": dict(envs_per_group=5), "zero groups": dict(groups=0), "unknown form": dict(form=4), "negative form": dict(form=-1),
             "unknown layout": dict(layout=2), "reset_rows 0": dict(reset_rows=0), "reset_rows 3": dict(reset_rows=3)}


def _bad_plan(kw):
    kw = dict(kw)
    raw, cells = kw.pop("raw", None), kw.pop("cells", [{}, {}])
    if len(cells) == 1:
        cells = cells + [{}]
    form, layout = kw.pop("form", scene.VARIANT_TT), kw.pop("layout", SOA)
    try:
        plan, arr = ssb.host_plan(12, cells, form, layout, **kw)
    except ValueError:                                   # the Python layer refuses a tilt beyond the series itself: go below it
        resolved = serve.resolve_cells([{}, {}], ssb.DEFAULTS, serve.AXES_27DOF)
        for axis, v in cells[0].items():
            resolved[0][axis] = v
        arr = serve.cell_structs(resolved)
        plan = _lib.ServePlan(num_envs=12, env_id_offset=0, seed=1, form=form, layout=layout, reset_rows=1, groups=2, envs_per_group=6, paired=0,
                              cells=C.cast(arr, C.c_void_p))
    if raw is not None:
        setattr(arr[1], *raw)
    return plan, arr


@pytest.mark.parametrize("case", list(BAD_PLANS))
def test_upload_refuses(case):
    S = ssb.lib()
    good, garr = ssb.host_plan(12, [{}, {}], scene.VARIANT_TT, SOA)
    assert S.serve_shim_invalid(C.byref(good), garr) == 0
    plan, arr = _bad_plan(BAD_PLANS[case])
    assert S.serve_shim_invalid(C.byref(plan), arr) != 0
    # ... and the library's own entry: it validates before it touches the device, so the pointers are never followed
    L = _lib.lib()
    fake = C.c_void_p(0x1000)
    assert L.pp_serve_plan_upload(C.byref(plan), arr, fake, fake, None) == EINVAL
    assert L.ppenv_last_error().decode().startswith("pp_serve_plan_upload: ")
    assert L.pp_serve_plan_upload(None, arr, fake, fake, None) == EINVAL and L.pp_serve_plan_upload(C.byref(good), garr, None, fake, None) == EINVAL


def test_launches_refuse_null_and_sizes():
    L, P = _lib.lib(), C.c_void_p(0x1000)
    assert L.pp_serve_fill(None, 4, P, P, None) == EINVAL and L.pp_serve_fill(P, 0, P, P, None) == EINVAL and L.pp_serve_fill(P, 4, None, P, None) == EINVAL
    assert L.pp_serve_apply(P, 4, None, P, P, None) == EINVAL and L.pp_serve_apply(P, -1, P, P, P, None) == EINVAL and L.pp_serve_apply(P, 4, P, P, None, None) == EINVAL
    assert L.pp_serve_apply_ids(P, 4, None, 2, P, P, None) == EINVAL and L.pp_serve_apply_ids(P, 4, P, -1, P, P, None) == EINVAL
    assert L.ppenv_last_error().decode().startswith("pp_serve_apply_ids: ")
    assert L.pp_serve_apply_ids(P, 4, None, 0, P, P, None) == 0                  # nothing listed: nothing launched
    assert not [n for n in vars(L) if n.startswith("ppenv_serve_plan") or n.startswith("ppenv_serve_apply")]     # the pinned ppenv_* set is untouched


def test_python_cells_and_sweep_axes():
    from isaacgym_amd.play import Sweep
    sw = Sweep.parse(["serve_speed=7.5:9:4", "serve_tilt=-5,-2.5,0", "friction_scale=0.5,1.0"])
    assert len(sw) == 24 and not sw.paired
    assert sw.cells[0] == {"serve_speed": 7.5, "serve_tilt": -5.0, "friction_scale": 0.5} and sw.cells[-1]["serve_speed"] == 9.0
    assert sorted(sw.tables({"friction_scale": 0, "link_mass_scale": 7}, 48)) == ["friction_scale"]              # the tables know no serve axis
    seven = {"serve_speed": (8.0, 8.6), "serve_tilt": (-5.0, 5.0), "serve_tilt_z": (2.0, 10.0)}
    cells = sw.serve_cells(seven)
    assert len(cells) == 24 and cells[0] == {"serve_speed": (7.5, 7.5), "serve_tilt": (-5.0, -5.0), "serve_tilt_z": (2.0, 10.0)}
    ranged = Sweep([{"serve_speed": (6.0, 6.5)}, {"serve_tilt_z": -4}], paired=True)
    assert ranged.paired and ranged.cells == [{"serve_speed": (6.0, 6.5)}, {"serve_tilt_z": -4.0}]
    assert ranged.serve_cells(seven)[1] == {"serve_speed": (8.0, 8.6), "serve_tilt": (-5.0, 5.0), "serve_tilt_z": (-4.0, -4.0)}
    # table-only sweeps: no plan unless paired, and then the configured ranges for every group
    plain = Sweep.grid({"friction_scale": [0.5, 1.0]})
    assert plain.serve_cells(seven) is None
    assert Sweep.grid({"friction_scale": [0.5, 1.0]}, paired=True).serve_cells(seven) == [seven, seven]
    assert Sweep.parse(["friction_scale=0.5,1.0"], paired=True).paired
    # refusals
    with pytest.raises(ValueError, match="serve axes are serve_speed, serve_tilt, serve_tilt_z$"):
        Sweep.parse(["ball_y=-0.2,0.0"]).serve_cells(seven)
    assert Sweep.parse(["ball_y=-0.2,0.0"]).serve_cells(dict(seven, ball_y=(-0.5, 0.1), ball_z=(0.96, 1.05)))[0]["ball_y"] == (-0.2, -0.2)
    with pytest.raises(ValueError, match="twice"):
        Sweep.parse(["serve_speed=7,8", "serve_speed=9"])
    for bad in ({"serve_tilt": 58.0}, {"serve_tilt_z": (-60.0, 0.0)}, {"serve_speed": (7.0, 6.0)}, {"serve_speed": float("nan")}, {"serve_speed": (1.0, 2.0, 3.0)},
                {"serve_speed[0]": 7.0}, {"friction_scale": -0.5}):
        with pytest.raises(ValueError):
            Sweep([bad])
    with pytest.raises(ValueError, match="multiple of 3 envs"):
        serve.ServePlan(None, "cpu", 10, [{}, {}, {}], seven, serve.AXES_7DOF, None, 1, 0, 1, 0)


def test_cli_paired_needs_sweep():
    from isaacgym_amd.play import parse_args
    a = parse_args(["--checkpoint", "x.pth", "--sweep", "serve_speed=7.5:9:4", "--sweep", "friction_scale=0.5,1.0", "--paired", "--sweep-out", "cells.json"])
    assert a.paired and a.sweep == ["serve_speed=7.5:9:4", "friction_scale=0.5,1.0"]
    assert not parse_args(["--checkpoint", "x.pth"]).paired
    for bad in (["--paired"], ["--sweep", "ball_x=1,2"], ["--sweep", "serve_tilt=0:70:3"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "x.pth"] + bad)


def test_group_summary_carries_paired():
    from isaacgym_amd.play import cell_text, group_summary
    tot = dict(games=0, steps=0, launches=0, reward=[0.0], reward_sq=[0.0], reward_min=[float("inf")], reward_max=[float("-inf")])
    assert group_summary({"serve_speed": 7.5}, tot, 1, 5, True)["paired"] is True and group_summary({}, tot, 1, 5)["paired"] is False
    assert cell_text({"serve_speed": (6.0, 6.5), "friction_scale": 0.5}) == "serve_speed=6..6.5 friction_scale=0.5"


# ------------------------------------------------------------------------------------------------------ 5. streams
def serves_seed(seed):
    return scene.stream_seed(seed, scene.STREAM_SERVES)


def lattice(kseed, keys):
    """uniform-level streams of the keys under one stream seed: counts 0, 1 x draws 0, 1, 2 -> [n, 6] 24-bit ints"""
    ep, k = np.repeat([0, 1], 3)[None, :], np.tile([0, 1, 2], 2)[None, :]
    return ubits(kseed, np.asarray(keys, U32)[:, None], ep, k)


def test_stream_salt_is_a_fourth_family():
    salts = [scene.STREAM_ENV, scene.STREAM_TABLES, scene.STREAM_SAMPLER, scene.STREAM_SERVES]
    assert len(set(salts)) == 4 and all(0 < s < 2 ** 64 for s in salts)
    for seed in (0, 1, 42, 2 ** 64 - 1):
        assert len({seed} | {scene.stream_seed(seed, s) for s in salts}) == 5


@pytest.mark.parametrize("seed", [0, 42, 4095])
def test_serve_plan_draws_share_none_with_the_other_families(seed):
    g = np.arange(64)
    env, tables = vec_task.VecTask.native_seeds({"seed": seed})
    mine = lattice(serves_seed(seed), g)
    others = {"env serve": lattice(env, g), "noise": lattice(env ^ NOISE_SALT, g), "tables": lattice(tables ^ scene.DR_SEED_SALT, g),
              "sampler": lattice(policy.sampler_stream_seed(seed) ^ NOISE_SALT, g)}
    for name, lat in others.items():
        assert shared(mine, lat) == 0, name
    # at the level of single 48-bit draw pairs, over more counts and keys
    def pairs(kseed, episodes, ks):
        gg, ee, kk = np.meshgrid(g.astype(U32), np.asarray(episodes, U32), np.asarray(ks, U32), indexing="ij")
        return (ubits(kseed, gg, ee, 2 * kk).astype(U64) << U64(24) | ubits(kseed, gg, ee, 2 * kk + U32(1)).astype(U64)).ravel()
    p = pairs(serves_seed(seed), range(16), [0, 1, 2])
    assert len(np.unique(p)) == p.size
    for kseed, eps, ks in ((env, [0, 1], [0, 1]), (env ^ NOISE_SALT, [0, 1], [q * 256 + 2 * j for q in range(8) for j in range(48)]),
                           (tables ^ scene.DR_SEED_SALT, [0, 1], np.arange(160)), (policy.sampler_stream_seed(seed) ^ NOISE_SALT, [0], [c * 256 + 2 * j for c in range(8) for j in range(14)])):
        assert np.intersect1d(p, pairs(kseed, eps, ks)).size == 0


def test_seeds_and_shards_share_no_serve_stream():
    n = 64
    g0, g1 = np.arange(n), n + np.arange(n)
    assert shared(lattice(serves_seed(42), g0), lattice(serves_seed(43), g0)) == 0
    assert shared(lattice(serves_seed(42), g0), lattice(serves_seed(42), g1)) == 0
    assert shared(lattice(serves_seed(42), g0), lattice(serves_seed(43), g1)) == 0
    # ... through the host build: two shards of one seed are the two halves of the single handle, and share nothing with each other
    def streams(h):
        a = h.out.T.copy()
        h.apply(np.ones(h.num_envs, np.int64))
        return np.concatenate([a, h.out.T], axis=1)
    cells = [{}]
    whole = streams(ssb.HostServe(2 * n, cells, scene.VARIANT_TT, SOA, seed=serves_seed(42)))
    lo, hi = streams(ssb.HostServe(n, cells, scene.VARIANT_TT, SOA, seed=serves_seed(42))), streams(ssb.HostServe(n, cells, scene.VARIANT_TT, SOA, seed=serves_seed(42), env_id_offset=n))
    assert np.array_equal(bits(whole[:n]), bits(lo)) and np.array_equal(bits(whole[n:]), bits(hi))
    assert shared(lo, hi) == 0
    assert shared(lo, streams(ssb.HostServe(n, cells, scene.VARIANT_TT, SOA, seed=serves_seed(43)))) == 0


@pytest.mark.parametrize("layout", [SOA, AOS], ids=["soa3", "aos5"])
def test_paired_key_is_shared_by_every_group(layout):
    G, S = 3, 20
    n = G * S

    def streams(paired, off=0):
        h = ssb.HostServe(n, [{}] * G, scene.VARIANT_TN, layout, seed=serves_seed(7), env_id_offset=off, paired=paired)
        a = (h.out.T if layout == SOA else h.out).copy()
        h.apply(np.full(n, 2 ** 32, np.int64))
        return np.concatenate([a, h.out.T if layout == SOA else h.out], axis=1)
    p, u = streams(True), streams(False)
    for g in range(1, G):
        assert np.array_equal(bits(p[g * S:(g + 1) * S]), bits(p[:S]))            # env i of every group: the same balls, in the same order
        assert shared(p[:S], p[g * S:(g + 1) * S]) == S
        assert shared(u[:S], u[g * S:(g + 1) * S]) == 0                            # unpaired: every env its own
    assert np.array_equal(bits(streams(True, off=1000)), bits(p))                 # the paired key does not see the shard's offset
    assert shared(lattice(serves_seed(7), np.arange(S)), lattice(serves_seed(7), np.arange(n) % S)[S:2 * S]) == S
