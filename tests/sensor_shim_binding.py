"""ctypes binding of tests/csrc/libppenv_sensorshim.so — the sensor line of the HIP kernel (isaacgym_amd/csrc/ppenv_sensor_device.h) compiled
for the host and walked in the kernel's order, built the way train_delay_shim_binding.lib() builds the delay line's — and the case generator
the host and the GPU suite share (cases(), case_data(), run_reference()).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import itertools
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd import scene, sensor

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "sensor_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", name) for name in ("ppenv_sensor_device.h", "ppenv_play_delay_device.h", "ppenv_device.h")] + \
        [os.path.join(_HERE, "..", "include", name) for name in ("ppenv_sensor.h", "ppenv_play_delay.h", "ppenv_play_group.h", "ppenv_play.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_sensorshim.so")
_FLAGS = ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"]      # isaacgym_amd._lib.SOURCE_FLAGS["ppenv_sensor.hip"]
_lib = None
COMMAND, SENSING = 0, 1
CANARY = 0xDEADBEEF
PUSHES = 6
STREAM = scene.stream_seed(42, scene.STREAM_SENSOR)


class Consts(C.Structure):
    """pp_sensor_consts, declared here on its own (the tests of isaacgym_amd._lib.SensorConsts compare the two layouts)."""
    _fields_ = [("sigma_lo", C.c_float), ("sigma_hi", C.c_float), ("drop_lo", C.c_float), ("drop_hi", C.c_float), ("draw", C.c_int32), ("seed", C.c_uint64),
                ("env_id_offset", C.c_int32), ("key_period", C.c_int32), ("channel", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, _FLAGS)
        i32, i64, u64, vp = C.c_int32, C.c_int64, C.c_uint64, C.c_void_p
        L.sensor_shim_consts_ok.restype = i32
        L.sensor_shim_consts_ok.argtypes = [C.POINTER(Consts)]
        for fn in (L.sensor_shim_uniform, L.sensor_shim_rng_uniform):
            fn.restype = None
            fn.argtypes = [u64, i32, i32, vp, vp, vp, i64, vp]
        L.sensor_shim_box_muller.restype = L.sensor_shim_reset.restype = L.sensor_shim_push.restype = None
        L.sensor_shim_box_muller.argtypes = [vp, vp, i64, vp, vp]
        L.sensor_shim_reset.argtypes = [i32, vp, vp]
        L.sensor_shim_push.argtypes = [vp, i64, vp, i32, i32, i32, C.POINTER(Consts), vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def shim_uniform(seed, channel, part, keys, episodes, k, through_rng_uniform=False):
    key, n, k = (np.ascontiguousarray(v) for v in np.broadcast_arrays(*(np.asarray(v, np.uint32) for v in (keys, episodes, k))))
    out = np.empty(key.shape, np.float32)
    fn = lib().sensor_shim_rng_uniform if through_rng_uniform else lib().sensor_shim_uniform
    fn(int(seed), channel, part, _p(key), _p(n), _p(k), key.size, _p(out))
    return out


def shim_box_muller(u1, u2):
    u1, u2 = np.ascontiguousarray(u1, np.float32), np.ascontiguousarray(u2, np.float32)
    g0, g1 = np.empty_like(u1), np.empty_like(u1)
    lib().sensor_shim_box_muller(_p(u1), _p(u2), u1.size, _p(g0), _p(g1))
    return g0, g1


def phased(words, phase, fill=CANARY):
    """A flat uint32 buffer of `words` words that begins `phase` words past a 16-byte boundary, with 4 guard words on either side
    -> (the backing array, kept alive by the caller; the [words] view).  Everything is filled with `fill`."""
    back = np.full(words + 16, fill, np.uint32)
    at = (-(back.ctypes.data // 4)) % 4 + 4 + phase            # first word at a 16-byte boundary, one piece of guard, then the phase
    return back, back[at:at + words]


class HostLine:
    """isaacgym_amd.sensor.SensorLine in numpy, stepped by the kernel body on the CPU.  held sits between guard words; out is [rows, ld_out]
    at word phase `phase_out`, pre-filled with CANARY."""

    def __init__(self, rows, width, num_agents=1, sigma=0.0, drop=0.0, columns=None, hold_columns=None, seed=0, env_id_offset=0, key_period=0,
                 channel=SENSING, ld_out=None, phase_out=0):
        self.L = lib()
        self.rows, self.width, self.A = R, W, _ = int(rows), int(width), int(num_agents)
        self.draw = 0 if isinstance(sigma, np.ndarray) else 1
        if self.draw:
            (s_lo, s_hi), (d_lo, d_hi) = sensor.sigma_range("sigma", sigma), sensor.drop_range("drop", drop)
            self.sigma, self.drop = np.zeros(R, np.float32), np.zeros(R, np.float32)
        else:
            s_lo = s_hi = d_lo = d_hi = 0.0
            self.sigma, self.drop = np.array(sigma, np.float32).reshape(R), np.array(drop, np.float32).reshape(R)
        self.consts = Consts(s_lo, s_hi, d_lo, d_hi, self.draw, int(seed), env_id_offset, key_period, channel)
        assert self.L.sensor_shim_consts_ok(C.byref(self.consts)) == 1
        self.col_scale = np.ones(W, np.float32) if columns is None else np.ascontiguousarray(columns, np.float32)
        self.col_hold = np.ones(W, np.int32) if hold_columns is None else np.ascontiguousarray(hold_columns, np.int32)
        self.ld_out = W if ld_out is None else int(ld_out)
        self.age, self.episode = np.zeros(R, np.int32), np.zeros(R, np.int32)
        self._held_back, held = phased(R * W, 0)
        self.held = held.reshape(R, W)
        self._out_back, out = phased(R * self.ld_out, phase_out)
        self.out_full = out.reshape(R, self.ld_out)
        self.dropped = np.zeros(R, np.int32)

    def reset(self):
        self.L.sensor_shim_reset(self.rows, _p(self.age), _p(self.episode))

    def push(self, x, done=None):
        """x: a uint32 [rows, ld_in >= width] view with unit stride along the row; done: int64 [rows] or None.  -> the [rows, width] view of out (uint32)."""
        assert x.dtype == np.uint32 and x.shape[0] == self.rows and x.shape[1] >= self.width and x.strides[1] == 4 and x.strides[0] == 4 * x.shape[1]
        d = None if done is None else np.ascontiguousarray(done, np.int64)
        self.L.sensor_shim_push(_p(x), x.shape[1], None if d is None else _p(d), self.rows, self.A, self.width, C.byref(self.consts), _p(self.col_scale),
                                _p(self.col_hold), _p(self.sigma), _p(self.drop), _p(self.age), _p(self.episode), _p(self.held), _p(self.out_full), self.ld_out,
                                _p(self.dropped))
        return self.out_full[:, :self.width]

    def guards_intact(self):
        """Every word of the two backing buffers outside held [rows, W] and out [rows, :W] is still CANARY."""
        held, out = self.held.copy(), self.out_full[:, :self.width].copy()
        self.held[:], self.out_full[:, :self.width] = CANARY, CANARY
        ok = bool((self._held_back == CANARY).all() and (self._out_back == CANARY).all())
        self.held[:], self.out_full[:, :self.width] = held, out
        return ok


# ---- the cases both suites share
SHAPES = ((1, 1), (2, 2), (65, 1), (130, 2))                                    # (rows, A)
WIDTHS = (1, 2, 3, 7, 27, 80, 313, 512)
SCALE_KINDS, HOLD_KINDS, DROPS = ("zero", "one", "mixed"), ("none", "all", "tail"), (0.0, 0.5, 1.0)


def cases():
    """Every (rows x A, W, ld) once; the other parameters — the input's and the output's word phase, col_scale, col_hold, drop, draw,
    key_period, channel — cycle with coprime periods over the 64 cases, so every value of every parameter occurs (test_sensor_host checks
    that), each with many of the others'.  -> list of dicts."""
    out = []
    for i, ((rows, A), W, pad) in enumerate(itertools.product(SHAPES, WIDTHS, (0, 1))):
        N = rows // A
        out.append(dict(id=f"rows{rows}-A{A}-W{W}-ld{W + pad}", rows=rows, A=A, W=W, ld=W + pad, phase_in=(i // 2 + i) % 4, phase_out=(3 * i + i // 8) % 4,
                        scale=SCALE_KINDS[(i + i // 3) % 3], hold=HOLD_KINDS[(i // 2 + i // 7) % 3], drop=DROPS[(i + i // 5) % 3], draw=(i // 2 + i // 16) % 2,
                        key_period=(N // 2) * ((i // 4) % 2), channel=(i + i // 2 + i // 32) % 2, offset=1000 * (i % 5), index=i))
    return out


def case_data(case):
    """-> dict(xs: list of PUSHES uint32 [rows, ld] views at the case's input phase (their backing arrays kept in `keep`), dones: int64
    [PUSHES, rows], col_scale, col_hold, sigma, drop: the SensorLine arguments).  The words are random floats in +-4 with -0.0, NaNs with a
    payload, +-inf and a denormal sprinkled in; padding columns hold CANARY.  The done pattern restarts envs at push 0 (even envs), push 1
    (env % 4 == 1), push 3 (env % 4 == 2) and at pushes 3 and 4 running (env % 4 == 3), with the words 1, 2 and 2^32; agent 1's own word is
    sometimes set, which the rule ignores."""
    rows, A, W, ld = case["rows"], case["A"], case["W"], case["ld"]
    rng = np.random.default_rng(1000 + case["index"])
    specials = np.array([0x80000000, 0x7FC01234, 0xFFC0BEEF, 0x7F800000, 0xFF800000, 0x00000001], np.uint32)
    xs, keep = [], []
    for _ in range(PUSHES):
        v = rng.uniform(-4, 4, (rows, W)).astype(np.float32).view(np.uint32)
        v = np.where(rng.random((rows, W)) < 0.04, specials[rng.integers(0, len(specials), (rows, W))], v)
        back, flat = phased(rows * ld, case["phase_in"])
        x = flat.reshape(rows, ld)
        x[:, :W] = v
        xs.append(x)
        keep.append(back)
    N = rows // A
    env = np.arange(N)
    dones = np.zeros((PUSHES, N), np.int64)
    dones[0, env % 2 == 0] = 1
    dones[1, env % 4 == 1] = 2
    dones[3, env % 4 == 2] = 1 << 32
    dones[3, env % 4 == 3] = 1
    dones[4, env % 4 == 3] = 1
    dones = np.repeat(dones, A, axis=1)
    if A == 2:
        stray = (rng.random((PUSHES, N)) < 0.3) & (dones[:, 0::2] == 0)
        dones[:, 1::2][stray] = 1
    scale = dict(zero=np.zeros(W), one=np.ones(W), mixed=rng.choice([0.0, 0.0, 0.5, 1.0, 2.0], W))[case["scale"]].astype(np.float32)
    hold = dict(none=np.zeros(W), all=np.ones(W), tail=(np.arange(W) >= W - 3))[case["hold"]].astype(np.int32)
    d = case["drop"]
    if case["draw"]:
        sigma, drop = (0.0, 0.5), (0.5 * d, d)
    else:
        sigma, drop = rng.choice([0.0, 0.01, 1.0], rows).astype(np.float32), np.full(rows, d, np.float32)
    return dict(xs=xs, keep=keep, dones=dones, col_scale=scale, col_hold=hold, sigma=sigma, drop=drop)


def line_kwargs(case, data):
    return dict(num_agents=case["A"], sigma=data["sigma"], drop=data["drop"], columns=data["col_scale"], hold_columns=data["col_hold"], seed=STREAM,
                env_id_offset=case["offset"], key_period=case["key_period"], channel=case["channel"])


_REFERENCE = {}


def run_reference(case):
    """sensor.reference over the case's pushes, computed once and shared: -> list of PUSHES dicts(out float32 bits as uint32, s, g, mag,
    dropped, age, episode, sigma, drop, held as uint32), read-only."""
    if case["index"] not in _REFERENCE:
        data = case_data(case)
        ref = sensor.reference(case["rows"], case["W"], **line_kwargs(case, data))
        steps = []
        for t in range(PUSHES):
            out = ref.push(data["xs"][t].view(np.float32), data["dones"][t])
            step = dict(out=out.view(np.uint32).copy(), s=ref.s.copy(), g=ref.g.copy(), mag=ref.mag.copy(), dropped=ref.dropped.copy(), age=ref.age.copy(),
                        episode=ref.episode.copy(), sigma=ref.sigma.copy(), drop=ref.drop.copy(), held=ref.held.view(np.uint32).copy())
            for v in step.values():
                v.setflags(write=False)
            steps.append(step)
        _REFERENCE[case["index"]] = steps
    return _REFERENCE[case["index"]]


def compare(got, step, e_normal, where, hold=None):
    """One push's delivered words `got` (uint32 [rows, W]) against the reference's step: where s == 0 the words are equal; elsewhere
    |got - ref| <= |s| * e_normal + 2^-23 * mag, with non-finite references matched by class.  -> the worst |got - ref| / |s| seen over the
    noised finite elements (0.0 without any), for the tests that measure."""
    ref = step["out"]
    copy = step["s"] == 0
    assert np.array_equal(got[copy], ref[copy]), where
    noisy = ~copy
    g, r = got.view(np.float32)[noisy].astype(np.float64), ref.view(np.float32)[noisy].astype(np.float64)
    fin = np.isfinite(r)
    assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), where
    s, mag = np.abs(step["s"][noisy].astype(np.float64))[fin], step["mag"][noisy][fin]
    err = np.abs(g[fin] - r[fin])
    bound = s * e_normal + 2.0 ** -23 * mag
    assert (err <= bound).all(), (where, float((err / np.maximum(bound, 1e-300)).max()))
    return float((np.maximum(err - 2.0 ** -23 * mag, 0) / s).max()) if err.size else 0.0
