"""The sensor line's rule without a GPU (include/ppenv_sensor.h): the host build of the kernel's device header (tests/csrc/sensor_shim.cpp)
against isaacgym_amd.sensor.reference on the cases the GPU suite shares, the consequences the header states, the column and range
parsers, scene.sensor_draws, and the ABI's refusals through the real library (argument validation alone: no device call)."""
import ctypes as C
import math

import numpy as np
import pytest

import sensor_shim_binding as sb
from isaacgym_amd import _lib, scene, sensor

# The host build's Box-Muller (libm in fp32: the angle 6.2831853f * u2 is rounded before cosf / sinf see it) against Box-Muller in fp64 on
# the same uniforms, in units of a standard normal: the worst over the 64 shared cases' noised elements, MEASURED here on the CPU by
# test_shim_equals_the_reference (which prints it), as tests/test_rng_streams_gpu.py measured the device's 5.03e-7.  Asserted at 4 x.
E_HOST_MEASURED = 1.37e-6
EINVAL = -1
CASES = sb.cases()


def test_the_cases_cover_every_value_the_suites_name():
    assert len(CASES) == 64 and {(c["rows"], c["A"]) for c in CASES} == set(sb.SHAPES) and {c["W"] for c in CASES} == set(sb.WIDTHS)
    for key, values in (("phase_in", range(4)), ("phase_out", range(4)), ("scale", sb.SCALE_KINDS), ("hold", sb.HOLD_KINDS), ("drop", sb.DROPS), ("draw", (0, 1)),
                        ("channel", (0, 1))):
        assert {c[key] for c in CASES} == set(values), key
        for W in sb.WIDTHS:
            assert len({c[key] for c in CASES if c["W"] == W}) >= 2, (key, W)
    assert {c["ld"] - c["W"] for c in CASES} == {0, 1}
    assert any(c["key_period"] == 0 for c in CASES) and any(c["key_period"] == c["rows"] // c["A"] // 2 > 0 for c in CASES)
    assert {(c["W"] % 2, c["phase_in"] % 2) for c in CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_the_uniforms_are_rng_uniform_bit_for_bit():
    """pp::sensor_uniform(pp::sensor_chain(...)) == rng_uniform of ppenv_device.h == scene.sensor_uniform, on keys up to 2^32 - 1."""
    rng = np.random.default_rng(3)
    key, n, k = (rng.integers(0, 2 ** 32, 4096, dtype=np.uint64) for _ in range(3))
    key[:4], n[:4], k[:4] = (0, 1, 2 ** 32 - 1, 7), (0, 0, 2 ** 32 - 1, 1), (0, 1, 2 ** 32 - 1, 2 ** 32 - 2)
    for channel in (0, 1):
        for part in (0, 1, 2):
            a = sb.shim_uniform(sb.STREAM, channel, part, key, n, k)
            assert np.array_equal(a, sb.shim_uniform(sb.STREAM, channel, part, key, n, k, through_rng_uniform=True))
            assert np.array_equal(a, scene.sensor_uniform(sb.STREAM, channel, part, key, n, k))
            assert a.min() >= 0 and a.max() < 1
    six = [sb.shim_uniform(sb.STREAM, ch, part, key, n, k) for ch in (0, 1) for part in (0, 1, 2)]
    assert all(not np.array_equal(six[i], six[j]) for i in range(6) for j in range(i))       # six streams, no two alike


@pytest.fixture(scope="module")
def shim_runs():
    """Every shared case through the host build, once: {index: (per push dicts, the guards' verdict)}."""
    runs = {}
    for case in CASES:
        data = sb.case_data(case)
        h = sb.HostLine(case["rows"], case["W"], ld_out=case["ld"], phase_out=case["phase_out"], **sb.line_kwargs(case, data))
        steps = []
        for t in range(sb.PUSHES):
            before = [x.copy() for x in data["keep"]]
            out = h.push(data["xs"][t], data["dones"][t])
            assert all(np.array_equal(a, b) for a, b in zip(before, data["keep"]))                # the input, its padding and guards are not modified
            steps.append(dict(out=out.copy(), age=h.age.copy(), episode=h.episode.copy(), sigma=h.sigma.copy(), drop=h.drop.copy(), dropped=h.dropped.copy(),
                              held=h.held.copy()))
        runs[case["index"]] = (steps, h.guards_intact())
    return runs


def test_shim_equals_the_reference(shim_runs):
    """age, episode, the drawn sigma / drop, every drop decision and every s == 0 column bit-exact; the noised values within
    |s| * 4 * E_HOST_MEASURED + 2^-23 * (|in| + |s g|); held likewise (it is what was delivered); canaries intact."""
    worst = 0.0
    for case in CASES:
        steps, guards = shim_runs[case["index"]]
        ref = sb.run_reference(case)
        for t in range(sb.PUSHES):
            where = (case["id"], t)
            for key in ("age", "episode"):
                assert np.array_equal(steps[t][key], ref[t][key]), (where, key)
            for key in ("sigma", "drop"):
                assert np.array_equal(steps[t][key].view(np.uint32), ref[t][key].view(np.uint32)), (where, key)
            assert np.array_equal(steps[t]["dropped"] != 0, ref[t]["dropped"]), where
            worst = max(worst, sb.compare(steps[t]["out"], ref[t], 4 * E_HOST_MEASURED, where))
            hold = np.broadcast_to(sb.case_data(case)["col_hold"] != 0, ref[t]["held"].shape) if t == sb.PUSHES - 1 else None
            if hold is not None:                                                               # the state at the end: only hold columns were ever written
                assert (steps[t]["held"][~hold] == sb.CANARY).all(), where
        assert guards, case["id"]
    print(f"host Box-Muller against fp64: worst {worst:.3e} of a unit normal (E_HOST_MEASURED {E_HOST_MEASURED:.3e})")
    assert worst <= E_HOST_MEASURED * 1.0001                                                   # the number written above IS the measured one


def test_box_muller_host_build_against_fp64():
    """sensor_box_muller on a grid of uniforms, the clamp at u1 = 0 included: within 4 x E_HOST_MEASURED of fp64, both branches."""
    rng = np.random.default_rng(5)
    u1 = np.concatenate([[0.0, 2.0 ** -24, 1 - 2.0 ** -24], rng.integers(0, 2 ** 24, 20000) * 2.0 ** -24]).astype(np.float32)
    u2 = np.concatenate([[0.0, 0.5, 1 - 2.0 ** -24], rng.integers(0, 2 ** 24, 20000) * 2.0 ** -24]).astype(np.float32)
    g0, g1 = sb.shim_box_muller(u1, u2)
    rad = np.sqrt(-2.0 * np.log(np.maximum(u1.astype(np.float64), 2.0 ** -24)))
    for got, want in ((g0, rad * np.cos(2 * np.pi * u2.astype(np.float64))), (g1, rad * np.sin(2 * np.pi * u2.astype(np.float64)))):
        assert np.abs(got - want).max() <= 4 * E_HOST_MEASURED + 2.0 ** -23 * np.abs(want).max()


def _line(rows, W, A=1, **kw):
    return sb.HostLine(rows, W, num_agents=A, seed=sb.STREAM, **kw)


def _words(rng, rows, W):
    return rng.uniform(-2, 2, (rows, W)).astype(np.float32).view(np.uint32)


def test_a_zero_row_is_a_bitwise_copy_and_draw_0_never_writes_the_table():
    rng = np.random.default_rng(7)
    rows, W = 9, 11
    sigma, drop = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
    sigma[::2], drop[1::3] = 0.3, 0.5
    h = _line(rows, W, sigma=sigma, drop=drop)
    x = _words(rng, rows, W)
    x[:, 3], x[:, 4] = 0x80000000, 0x7FC01234
    for t in range(5):
        out = h.push(x)
        quiet = (sigma == 0) & (drop == 0)
        assert np.array_equal(out[quiet], x[quiet])
        assert not np.array_equal(out[sigma > 0], x[sigma > 0])
        assert np.array_equal(h.sigma, sigma) and np.array_equal(h.drop, drop)


def test_nothing_crosses_a_reset_and_the_first_sample_is_never_dropped():
    """drop = 1, sigma = 0, every column held: an episode delivers its first sample for ever; a done word starts the next episode with ITS first
    sample; a dropped sample delivers what was delivered, noise included, bit for bit."""
    rng = np.random.default_rng(9)
    rows, W, A = 6, 5, 2
    h = _line(rows, W, A, sigma=np.zeros(rows, np.float32), drop=np.ones(rows, np.float32))
    xs = [_words(rng, rows, W) for _ in range(6)]
    done = np.zeros(rows, np.int64)
    first = xs[0].copy()
    for t in range(6):
        done[:] = 0
        if t == 3:
            done[2] = 1 << 40                                    # env 1's agent 0: rows 2 and 3 restart
            done[5] = 1                                          # env 2's agent 1 alone: ignored
            first[2:4] = xs[3][2:4]
        out = h.push(xs[t], None if t == 0 else done)
        assert np.array_equal(out, first), t
        assert np.array_equal(h.dropped != 0, np.array([t > 0] * rows) & ~np.isin(np.arange(rows), (2, 3) if t == 3 else ())), t
    assert list(h.episode) == [1, 1, 2, 2, 1, 1] and list(h.age) == [6, 6, 3, 3, 6, 6]
    noisy = _line(rows, W, A, sigma=np.full(rows, 0.5, np.float32), drop=np.ones(rows, np.float32))
    a = noisy.push(xs[0]).copy()
    assert not np.array_equal(a, xs[0])
    assert np.array_equal(noisy.push(xs[1]), a) and np.array_equal(noisy.push(xs[2]), a)
    tail = _line(rows, W, A, sigma=np.zeros(rows, np.float32), drop=np.ones(rows, np.float32), hold_columns=np.array([0, 0, 0, 1, 1]))
    tail.push(xs[0])
    out = tail.push(xs[1])
    assert np.array_equal(out[:, :3], xs[1][:, :3]) and np.array_equal(out[:, 3:], xs[0][:, 3:])      # only the hold columns freeze
    assert (tail.held[:, :3] == sb.CANARY).all()                                                       # held is touched only for hold columns


@pytest.mark.parametrize("draw", (0, 1))
def test_two_shards_with_offsets_equal_one_handle(draw):
    rng = np.random.default_rng(11)
    rows, W, A, off = 24, 7, 2, 500
    N, cut = rows // A, 10
    sigma, drop = ((0.0, 0.4), (0.1, 0.6)) if draw else (rng.uniform(0, 1, rows).astype(np.float32), rng.uniform(0, 0.7, rows).astype(np.float32))
    part = lambda v, a, b: v if draw else v[a:b]
    whole = _line(rows, W, A, sigma=sigma, drop=drop, env_id_offset=off)
    lo = _line(cut, W, A, sigma=part(sigma, 0, cut), drop=part(drop, 0, cut), env_id_offset=off)
    hi = _line(rows - cut, W, A, sigma=part(sigma, cut, rows), drop=part(drop, cut, rows), env_id_offset=off + cut // A)
    for t in range(8):
        x = _words(rng, rows, W)
        done = np.repeat((rng.random(N) < 0.3).astype(np.int64), A)
        out = whole.push(x, done).copy()
        a, b = lo.push(np.ascontiguousarray(x[:cut]), done[:cut]), hi.push(np.ascontiguousarray(x[cut:]), done[cut:])
        assert np.array_equal(out, np.concatenate([a, b])), t
        for key in ("age", "episode", "sigma", "drop", "dropped"):
            assert np.array_equal(getattr(whole, key), np.concatenate([getattr(lo, key), getattr(hi, key)])), (t, key)


def test_paired_halves_see_the_same_standard_normals():
    """key_period = S: env e and env e + S deliver (out - in) bitwise equal at equal sigma and equal input, drop decisions included; at
    another sigma the drop decisions are still equal and the normals the reference reads back are."""
    rng = np.random.default_rng(13)
    S, W, A = 8, 9, 2
    rows = 2 * S * A
    half = A * S
    sigma, drop = np.full(rows, 0.25, np.float32), np.full(rows, 0.4, np.float32)
    h = _line(rows, W, A, sigma=sigma, drop=drop, key_period=S, env_id_offset=77)
    plain = _line(rows, W, A, sigma=sigma, drop=drop, env_id_offset=77)
    for t in range(6):
        x = np.tile(_words(rng, half, W), (2, 1))
        done = np.tile(np.repeat((rng.random(S) < 0.3).astype(np.int64), A), 2)
        out = h.push(x, done).view(np.float32) - x.view(np.float32)
        assert np.array_equal(out[:half].view(np.uint32), out[half:].view(np.uint32)) and np.array_equal(h.dropped[:half], h.dropped[half:]), t
        other = plain.push(x, done).view(np.float32) - x.view(np.float32)
        assert np.array_equal(other[:half], out[:half]) and not np.array_equal(other[half:], out[half:]), t     # without the period: other keys
    sigma2 = sigma.copy()
    sigma2[half:] = 0.75
    r = sensor.reference(rows, W, A, sigma=sigma2, drop=drop, key_period=S, env_id_offset=77, seed=sb.STREAM)
    r.push(np.zeros((rows, W), np.float32))
    assert np.array_equal(r.g[:half], r.g[half:]) and np.abs(r.out[half:] / 0.75 - r.out[:half] / 0.25).max() < 1e-6      # s * g scales with sigma


def test_sensor_draws_predicts_the_level_draws():
    rows, W, A, off = 20, 3, 2, 300
    rng = np.random.default_rng(17)
    for channel in (0, 1):
        h = _line(rows, W, A, sigma=(0.01, 0.3), drop=(0.0, 0.5), env_id_offset=off, channel=channel)
        for t in range(10):
            done = np.repeat((rng.random(rows // A) < 0.4).astype(np.int64), A)
            h.push(_words(rng, rows, W), done)
            r = np.arange(rows)
            for agent in range(A):
                rr = r[agent::A]
                sg, dp = scene.sensor_draws(sb.STREAM, off + rr // A, h.episode[rr] - 1, channel, (0.01, 0.3), (0.0, 0.5), num_agents=A, agent=agent)
                assert np.array_equal(sg, h.sigma[rr]) and np.array_equal(dp, h.drop[rr]), (channel, t, agent)
        assert h.sigma.min() >= np.float32(0.01) and h.sigma.max() <= np.float32(0.3) and len(set(h.sigma)) > rows // 2
        assert h.episode.max() > 2
    fixed = _line(rows, W, A, sigma=0.125, drop=0.25)
    fixed.push(_words(rng, rows, W))
    assert (fixed.sigma == 0.125).all() and (fixed.drop == 0.25).all()                     # lo == hi gives lo for every key
    for kw in (dict(sigma=(-1, 0)), dict(sigma=(2, 1)), dict(drop=(0, 1.5)), dict(channel=2), dict(num_agents=3), dict(agent=1)):
        a = dict(sigma=(0, 1), drop=(0, 1), channel=0)
        a.update(kw)
        channel = a.pop("channel")
        with pytest.raises(ValueError, match="sensor_draws"):
            scene.sensor_draws(1, [0], [0], channel, **a)


def test_the_column_parser():
    cols, hold = sensor.columns, sensor.hold_columns
    for variant in ("TT", "T4", "T3", "TN"):
        c = cols(variant, "ball_pos=1,ball_vel=4,60:67=0.5", 80)
        assert c.dtype == np.float32 and list(np.flatnonzero(c)) == list(range(60, 67)) + list(range(74, 80))
        assert (c[74:77] == 1).all() and (c[77:80] == 4).all() and (c[60:67] == 0.5).all()
    assert sensor.groups("TT") == dict(body_pos=(0, 30), body_vel=(30, 60), dof_pos=(60, 67), dof_vel=(67, 74), ball_pos=(74, 77), ball_vel=(77, 80))
    assert sum(hi - lo for lo, hi in sensor.groups("TT").values()) == scene.NUM_OBS == 80
    assert sensor.groups("TA") == {} and sensor.groups("TT", sensor.COMMAND) == {}

    class Task:
        VARIANT = "T4"
    assert np.array_equal(cols(Task(), "ball_pos", 80), cols("TT", "74:77=1", 80))
    assert (cols("TA", None, 313) == 1).all() and (cols("TA", "", 313) == 1).all() and (cols("TA", "all=0.25", 313) == 0.25).all()
    assert np.array_equal(cols("TA", "all=2, 0:3=0", 313), np.r_[np.zeros(3), np.full(310, 2.0)].astype(np.float32))      # left to right
    h = hold("TT", "ball_pos,ball_vel", 80)
    assert h.dtype == np.int32 and list(np.flatnonzero(h)) == list(range(74, 80)) and (hold("TT", None, 80) == 1).all()
    assert list(np.flatnonzero(hold(None, "2:4", 7, sensor.COMMAND))) == [2, 3]
    for args, text in ((("TT", "ball=1", 80), "unknown column group 'ball'; the groups are all, body_pos, body_vel, dof_pos, dof_vel, ball_pos, ball_vel, or a range LO:HI"),
                       (("TA", "ball_pos", 313), "unknown column group 'ball_pos'; the groups are all, or a range LO:HI"),
                       (("TT", "ball_pos", 7, sensor.COMMAND), "unknown column group 'ball_pos'; the groups are all, or a range LO:HI"),
                       (("TT", "70:81", 80), "the range 70:81 is not inside 0:80 with LO < HI"), (("TT", "5:5", 80), "the range 5:5 is not inside 0:80"),
                       (("TT", "a:b", 80), "a range is LO:HI, two whole numbers"), (("TT", "1:2:3", 80), "a range is LO:HI, two whole numbers"),
                       (("TT", "ball_pos=-1", 80), "the scale '-1' is not a finite number >= 0"), (("TT", "ball_pos=nan", 80), "is not a finite number >= 0"),
                       (("TT", "ball_pos=x", 80), "the scale 'x' is not a finite number >= 0"), (("TT", "all", 0), "width 0 is outside 1..512"),
                       (("TT", "all", 513), "width 513 is outside 1..512"), (("TT", 3, 80), "a column spec is text")):
        with pytest.raises(ValueError, match="columns: ") as e:
            cols(*args)
        assert text in str(e.value), (args, str(e.value))
    with pytest.raises(ValueError, match="obs_drop_columns: 'ball_pos=2': these columns take no scale"):
        hold("TT", "ball_pos=2", 80, name="obs_drop_columns")


def test_the_range_parser():
    pr = sensor.parse_range
    assert pr("x", 0.5) == (0.5, 0.5) and pr("x", 2) == (2.0, 2.0) and pr("x", (0, 0.25)) == (0.0, 0.25) and pr("x", [0.1, 0.1]) == (0.1, 0.1)
    assert pr("x", "0.02") == (0.02, 0.02) and pr("x", "0:0.02") == (0.0, 0.02) and pr("x", " 1e-3 : 2e-3 ") == (0.001, 0.002)
    assert sensor.drop_range("p", "0.2:1") == (0.2, 1.0) and sensor.sigma_range("s", np.float32(3)) == (3.0, 3.0)
    for bad in (-0.1, (0.2, 0.1), "0.2:0.1", math.inf, math.nan, "x", "1:2:3", (1,), (1, 2, 3), True, None, {}, "nan"):
        with pytest.raises(ValueError, match="obs_noise: a number S or a range LO:HI / \\(lo, hi\\) with 0 <= lo <= hi, finite, not"):
            pr("obs_noise", bad)
    for bad in (1.5, (0, 1.0001), "0:2", -1):
        with pytest.raises(ValueError, match="obs_drop: a number S or a range LO:HI / \\(lo, hi\\) with 0 <= lo <= hi <= 1, finite, not"):
            sensor.drop_range("obs_drop", bad)


def test_the_binding_and_the_build_list():
    assert [(n, t) for n, t in _lib.SensorConsts._fields_] == [(n, t) for n, t in sb.Consts._fields_] and C.sizeof(_lib.SensorConsts) == 48
    assert _lib.SensorConsts.seed.offset == 24 and _lib.SensorConsts.channel.offset == 40
    assert any(p.endswith("ppenv_sensor.hip") for p in _lib.SOURCES) and sum(p.endswith(("ppenv_sensor.h", "ppenv_sensor_device.h")) for p in _lib.HEADERS) == 2
    assert _lib.SOURCE_FLAGS["ppenv_sensor.hip"] == ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"]
    assert scene.STREAM_SENSOR not in (scene.STREAM_ENV, scene.STREAM_TABLES, scene.STREAM_SAMPLER, scene.STREAM_SERVES, scene.STREAM_LATENCY)


def test_the_abi_refuses_before_any_device_call():
    """Through the real library's entries, with made-up non-NULL addresses that a launch would fault on: every refusal returns PPENV_EINVAL
    with its message before the HIP runtime is touched, so this passes on a machine without a GPU."""
    L = _lib.lib()
    rows, A, W = 8, 2, 5
    fake = 0x1000

    def push(consts=True, **kw):
        c = dict(sigma_lo=0.0, sigma_hi=1.0, drop_lo=0.0, drop_hi=1.0, draw=1, seed=1, env_id_offset=0, key_period=0, channel=0)
        a = dict(x=fake, ld_in=W, done=fake, rows=rows, A=A, W=W, col_scale=fake, col_hold=fake, sigma=fake, drop=fake, age=fake, episode=fake, held=fake, out=fake,
                 ld_out=W)
        c.update({k: v for k, v in kw.items() if k in c})
        a.update({k: v for k, v in kw.items() if k in a})
        cs = _lib.SensorConsts(**c)
        rc = L.pp_sensor_push(a["x"], a["ld_in"], a["done"], a["rows"], a["A"], a["W"], C.byref(cs) if consts else None, a["col_scale"], a["col_hold"], a["sigma"],
                              a["drop"], a["age"], a["episode"], a["held"], a["out"], a["ld_out"], None)
        return rc, L.ppenv_last_error().decode()

    cases = [(dict(consts=False), "NULL constants"), (dict(sigma_lo=-1.0), "sigma_lo -1, sigma_hi 1: need finite 0 <= lo <= hi"),
             (dict(sigma_lo=2.0), "sigma_lo 2, sigma_hi 1: need finite"), (dict(sigma_hi=math.inf), "sigma_hi inf"), (dict(sigma_hi=math.nan), "sigma_hi nan"),
             (dict(sigma_lo=math.nan), "need finite 0 <= lo <= hi"), (dict(drop_hi=1.5), "drop_lo 0, drop_hi 1.5: need 0 <= lo <= hi <= 1"),
             (dict(drop_lo=-0.5), "drop_lo -0.5"), (dict(drop_lo=0.75, drop_hi=0.5), "drop_lo 0.75, drop_hi 0.5"), (dict(drop_lo=math.nan), "need 0 <= lo <= hi <= 1"),
             (dict(draw=2), "draw 2 is not 0"), (dict(draw=-1), "draw -1 is not 0"), (dict(key_period=-1), "key_period -1"), (dict(env_id_offset=-3), "env_id_offset -3"),
             (dict(channel=2), "channel 2 is not 0 (command) or 1 (sensing)"), (dict(channel=-1), "channel -1")]
    cases += [(kw, "NULL pointer (done excepted)") for kw in (dict(x=None), dict(col_scale=None), dict(col_hold=None), dict(sigma=None), dict(drop=None), dict(age=None),
                                                              dict(episode=None), dict(held=None), dict(out=None), dict(rows=0), dict(rows=7), dict(A=0), dict(A=3),
                                                              dict(W=0), dict(W=513), dict(ld_in=W - 1), dict(ld_out=W - 1))]
    for kw, text in cases:
        rc, msg = push(**kw)
        assert rc == EINVAL and msg.startswith("pp_sensor_push: ") and text in msg, (kw, rc, msg)
    assert L.pp_sensor_reset(0, fake, fake, None) == EINVAL and L.ppenv_last_error().decode() == "pp_sensor_reset: NULL pointer or rows < 1"
    assert L.pp_sensor_reset(rows, None, fake, None) == EINVAL and L.pp_sensor_reset(rows, fake, None, None) == EINVAL
    assert L.pp_sensor_table_bytes(rows) == 4 * rows and L.pp_sensor_held_bytes(rows, W) == 4 * rows * W
    assert L.pp_sensor_table_bytes(0) == 0 and L.pp_sensor_held_bytes(0, W) == 0 and L.pp_sensor_held_bytes(rows, 0) == 0 and L.pp_sensor_held_bytes(rows, 513) == 0
    ok = sb.Consts(0.0, 1.0, 0.0, 1.0, 1, 1, 0, 0, 0)
    assert sb.lib().sensor_shim_consts_ok(C.byref(ok)) == 1
    for field, v in (("sigma_lo", -1.0), ("sigma_hi", math.inf), ("drop_hi", 1.5), ("draw", 2), ("key_period", -1), ("env_id_offset", -1), ("channel", 2)):
        bad = sb.Consts(0.0, 1.0, 0.0, 1.0, 1, 1, 0, 0, 0)
        setattr(bad, field, v)
        assert sb.lib().sensor_shim_consts_ok(C.byref(bad)) == 0, field
