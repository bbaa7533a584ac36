"""The control-latency delay line (include/ppenv_play_delay.h) without a GPU: the kernel body on the host (tests/csrc/play_delay_shim.cpp)
against a numpy restatement of the header's rule on int32 views — odd widths, strides above the width, NaN payloads and -0.0, done on
the first push and on consecutive pushes —, the zero-delay identity, agent 1's done word, the C entries' refusals, and the Python side:
the sweep's latency axes, Sweep.delays, Delay's refusals, the CLI options; and the shim under the address and undefined-behaviour
sanitizers as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import play_delay_shim_binding as pd
from isaacgym_amd import _lib, play

EINVAL = -1
_HERE = os.path.dirname(os.path.abspath(__file__))


def i32(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------------- the shim against numpy
@pytest.mark.parametrize("shape", pd.SHAPES, ids=pd.shape_id)
def test_shim_equals_the_numpy_restatement(shape):
    rows, A = shape
    for W, depth, pad in pd.subcases():
        d = pd.case_delays(rows, depth)
        assert d.max() == depth - 1 and (rows == 1 or d.min() == 0)
        xs, dones = pd.case_stream(rows, A, W, depth, pad)
        assert len(xs) == 3 * depth + 5 and np.isnan(xs[..., :W].view(np.float32)).any() and (xs[..., :W] == 0x80000000).any()
        h, ref = pd.HostDelay(rows, W, d, A, ld_out=W + pad), pd.NumpyDelay(rows, W, d, A)
        for t in range(len(xs)):
            keep = xs[t].copy()
            got, want = h.push(xs[t], dones[t]), ref.push(xs[t], dones[t])
            what = (rows, A, W, depth, pad, t)
            assert np.array_equal(i32(got), i32(want)), what
            assert np.array_equal(xs[t], keep), what                                         # the input is not modified
            assert (h.out[:, W:] == pd.GARBAGE).all(), what                                  # ... nor the output's padding written
        assert np.array_equal(h.age, ref_age(dones, A)), (rows, A, W, depth, pad)


def ref_age(dones, A):
    """age after the stream: pushes since (and with) the last push whose done word was set, or all of them."""
    T = dones.shape[0]
    first = np.repeat(dones.reshape(T, -1, A)[:, :, 0] != 0, A, axis=1)
    last = np.where(first.any(0), T - 1 - np.argmax(first[::-1], axis=0), 0)
    return (T - last).astype(np.int32)


def test_first_push_without_done_and_a_reset_in_the_middle():
    """reset() then done = None is the start of an episode for every row; nothing is carried across a reset()."""
    rows, W, A = 65, 7, 1
    d = pd.case_delays(rows, 4)
    xs, dones = pd.case_stream(rows, A, W, 4, 0)
    h, ref = pd.HostDelay(rows, W, d, A), pd.NumpyDelay(rows, W, d, A)
    for part in (range(0, 9), range(9, len(xs))):
        h.reset()
        ref.reset()
        for k, t in enumerate(part):
            done = None if k == 0 else dones[t]
            assert np.array_equal(i32(h.push(xs[t], done)), i32(ref.push(xs[t], done))), t


def test_all_delays_zero_is_the_identity_on_every_push():
    for rows, A, W in ((130, 2, 27), (65, 1, 313), (1, 1, 1)):
        xs, dones = pd.case_stream(rows, A, W, 2, 1)
        h = pd.HostDelay(rows, W, np.zeros(rows, np.int32), A, ld_out=W + 1)
        assert h.depth == 1
        for t in range(len(xs)):
            assert np.array_equal(i32(h.push(xs[t], dones[t])), i32(xs[t][:, :W]))


def test_a_delay_holds_the_first_sample_then_lags_by_exactly_d():
    rows, W, dmax = 4, 3, 3
    d = np.array([0, 1, 2, 3], np.int32)
    h = pd.HostDelay(rows, W, d)
    xs = (np.arange(10 * rows * W, dtype=np.uint32) + 1).reshape(10, rows, W)
    for t in range(10):
        done = None if t == 0 else np.full(rows, 1 if t == 6 else 0, np.int64)                   # every env restarts at push 6
        out = h.push(xs[t], done)
        start = 6 if t >= 6 else 0
        for r in range(rows):
            assert np.array_equal(out[r], xs[max(t - d[r], start)][r]), (t, r)


def test_agent_1s_done_word_is_ignored():
    rows, W, A = 8, 5, 2
    d = np.full(rows, 2, np.int32)
    xs, _ = pd.case_stream(rows, A, W, 3, 0)
    a, b = pd.HostDelay(rows, W, d, A), pd.HostDelay(rows, W, d, A)
    for t in range(len(xs)):
        none = np.zeros(rows, np.int64)
        stray = none.copy()
        stray[1::2] = 1 << 32                                                                  # agent 1's rows only
        assert np.array_equal(a.push(xs[t], none), b.push(xs[t], stray))
    both = np.zeros(rows, np.int64)
    both[2] = 2                                                                                # agent 0 of env 1: both of its rows restart
    out = a.push(xs[0], both)
    assert np.array_equal(out[2:4], xs[0][2:4, :W]) and not np.array_equal(out[0:2], xs[0][0:2, :W])


def test_rows_per_workgroup():
    L = pd.lib()
    assert [L.play_delay_shim_rows_per_block(w) for w in (1, 4, 7, 27, 80, 313, 512)] == [256, 256, 146, 37, 12, 3, 2]


# ------------------------------------------------------------------------------------------------------- the C entries
PUSH_TEXT = ("pp_play_delay_push: NULL pointer (done excepted), rows < 1 or no multiple of num_agents, num_agents not 1 or 2, width outside 1..512, "
             "depth outside 1..16, or a stride below width")
RESET_TEXT = "pp_play_delay_reset: NULL pointer or rows < 1"
P = 0x1000                      # a non-NULL pointer value: a refusal comes before anything is read or launched


def _poison(L):
    assert L.ppenv_gae(*([None] * 2 + [0, 0, None, 0, 0, 0.0, 0.0, 0.0, None, None, None])) == EINVAL      # another text in ppenv_last_error()
    return L.ppenv_last_error().decode()


def _push(L, x=P, ld_in=7, done=P, rows=4, A=1, W=7, K=3, delay=P, age=P, ring=P, out=P, ld_out=7):
    return L.pp_play_delay_push(x, ld_in, done, rows, A, W, K, delay, age, ring, out, ld_out, None)


def test_entries_are_bound_on_the_default_library_and_on_one_loaded_by_path(tmp_path):
    import shutil
    i32_, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    for L in (_lib.lib(), _lib.load(str(shutil.copy(_lib.LIB_PATH, tmp_path / "libppenv_copy.so")))):
        assert L.pp_play_delay_ring_bytes.argtypes == [i32_, i32_, i32_] and L.pp_play_delay_ring_bytes.restype is C.c_size_t
        assert L.pp_play_delay_reset.argtypes == [i32_, vp, vp]
        assert L.pp_play_delay_push.argtypes == [vp, i64, vp, i32_, i32_, i32_, i32_, vp, vp, vp, vp, i64, vp]
    for name in ("ppenv_play_delay_reset", "ppenv_play_delay_push", "ppenv_play_delay_ring_bytes"):
        assert not hasattr(C.CDLL(_lib.LIB_PATH), name)                                  # the pinned set of ppenv_* symbols is untouched


def test_ring_bytes():
    L = _lib.lib()
    for rows, W, K in ((1, 1, 1), (130, 27, 16), (8192, 313, 3), (16384, 80, 16), (1 << 24, 512, 16)):
        assert L.pp_play_delay_ring_bytes(rows, W, K) == 4 * K * rows * W
    for rows, W, K in ((0, 7, 2), (-1, 7, 2), (4, 0, 2), (4, 513, 2), (4, 7, 0), (4, 7, 17), (4, -1, 2), (4, 7, -1)):
        assert L.pp_play_delay_ring_bytes(rows, W, K) == 0


@pytest.mark.parametrize("kw", [dict(rows=0), dict(rows=-4), dict(rows=5, A=2), dict(A=0), dict(A=3), dict(W=0, ld_in=0, ld_out=0), dict(W=513, ld_in=513, ld_out=513),
                                dict(K=0), dict(K=17), dict(K=-1), dict(ld_in=6), dict(ld_out=6), dict(ld_in=0), dict(ld_out=-7)], ids=str)
def test_push_refuses_sizes(kw):
    L = _lib.lib()
    assert _poison(L) != PUSH_TEXT
    assert _push(L, **kw) == EINVAL
    assert L.ppenv_last_error().decode() == PUSH_TEXT


@pytest.mark.parametrize("name", ["x", "delay", "age", "ring", "out"])
def test_push_refuses_null(name):
    L = _lib.lib()
    _poison(L)
    assert _push(L, **{name: None}) == EINVAL
    assert L.ppenv_last_error().decode() == PUSH_TEXT


@pytest.mark.parametrize("rows,age", [(0, P), (-1, P), (4, None)])
def test_reset_refuses(rows, age):
    L = _lib.lib()
    assert _poison(L) != RESET_TEXT
    assert L.pp_play_delay_reset(rows, age, None) == EINVAL
    assert L.ppenv_last_error().decode() == RESET_TEXT


# ------------------------------------------------------------------------------------------------------- the Python side
def test_delay_refusals():
    ok = dict(rows=8, width=7, delays=np.zeros(8, np.int32), device="cpu")
    for kw in (dict(rows=0), dict(rows=7, delays=np.zeros(7, np.int32), num_agents=2), dict(num_agents=3), dict(num_agents=0), dict(width=0), dict(width=513),
               dict(delays=np.zeros(7, np.int32)), dict(delays=np.zeros((8, 1), np.int32)), dict(delays=np.zeros(8, np.float32)),
               dict(delays=np.full(8, 16)), dict(delays=np.full(8, -1)), dict(delays=3)):
        with pytest.raises(ValueError, match="^Delay"):
            play.Delay(**dict(ok, **kw))


def test_sweep_parses_the_latency_axes():
    sw = play.Sweep.parse(["action_delay=0:3:4"])
    assert sw.cells == [{"action_delay": k} for k in range(4)] and all(type(c["action_delay"]) is int for c in sw.cells)
    sw = play.Sweep.parse(["action_delay=0,2.0", "obs_delay=1"], paired=True)
    assert sw.cells == [{"action_delay": 0, "obs_delay": 1}, {"action_delay": 2, "obs_delay": 1}] and sw.paired
    assert play.Sweep([{"obs_delay": np.int64(15)}, {"obs_delay": 3.0}]).cells == [{"obs_delay": 15}, {"obs_delay": 3}]
    assert play.cell_text(sw.cells[1]) == "action_delay=2 obs_delay=1"
    for spec in ("action_delay=1.5", "action_delay=0:3:3", "action_delay=16", "obs_delay=-1", "obs_delay=0,0.5"):
        with pytest.raises(ValueError, match=rf"{spec.split('=')[0]}.*whole control steps"):
            play.Sweep.parse([spec])
    for v in ((0, 2), [1, 2], 1.5, 16, -1, float("nan"), float("inf"), "2", True, None):
        with pytest.raises(ValueError, match="'action_delay'.*whole control steps"):
            play.Sweep([{"action_delay": v}])
    with pytest.raises(ValueError, match="serve axis: serve_speed, serve_tilt, serve_tilt_z, ball_y, ball_z, or a latency axis in whole control steps: action_delay, obs_delay$"):
        play.Sweep([{"act_delay": 1}])
    with pytest.raises(ValueError, match="dof_stiffness_scale, dof_damping_scale, link_mass_scale, restitution_scale, friction_scale, or one row of a table"):
        play.Sweep.parse(["action_delay[0]=1"])


def test_tables_and_serve_cells_are_blind_to_the_latency_axes():
    sw = play.Sweep.grid({"action_delay": [0, 2], "friction_scale": [0.5, 1.0], "obs_delay": [1]})
    plain = play.Sweep.grid({"friction_scale": [0.5, 1.0, 0.5, 1.0]})
    rows = {"friction_scale": 0, "link_mass_scale": 7}
    got, want = sw.tables(rows, 48), plain.tables(rows, 48)
    assert sorted(got) == ["friction_scale"] and np.array_equal(got["friction_scale"], want["friction_scale"])
    assert play.Sweep.grid({"action_delay": [0, 2]}).tables(rows, 48) == {}
    defaults = {"serve_speed": (7.0, 9.0), "serve_tilt": (-3.0, 3.0), "serve_tilt_z": (-1.0, 1.0)}
    assert sw.serve_cells(defaults) is None
    paired = play.Sweep.grid({"action_delay": [0, 2], "serve_speed": [8.0]}, paired=True)
    assert paired.serve_cells(defaults) == play.Sweep([{"serve_speed": 8.0}] * 2, paired=True).serve_cells(defaults)


def test_sweep_delays_layout():
    sw = play.Sweep([{"action_delay": 2}, {"obs_delay": 1}, {"action_delay": 3, "obs_delay": 15}])
    d = sw.delays(12, 2)                                                                   # S = 4 envs, 8 rows per cell
    assert set(d) == {"action_delay", "obs_delay"} and all(v.dtype == np.int32 and v.shape == (24,) for v in d.values())
    assert d["action_delay"].tolist() == [2] * 8 + [0] * 8 + [3] * 8 and d["obs_delay"].tolist() == [0] * 8 + [1] * 8 + [15] * 8
    d = sw.delays(12, 2, action_delay=5, obs_delay=4)                                      # the keywords fill the cells that do not name the axis
    assert d["action_delay"].tolist() == [2] * 8 + [5] * 8 + [3] * 8 and d["obs_delay"].tolist() == [4] * 8 + [1] * 8 + [15] * 8
    assert sw.delays(3, 1)["action_delay"].tolist() == [2, 0, 3]
    assert sw.cell_delays(obs_delay=4) == dict(action_delay=[2, 0, 3], obs_delay=[4, 1, 15])
    with pytest.raises(ValueError, match="multiple of 3 envs, not 8"):
        sw.delays(8, 2)
    with pytest.raises(ValueError, match="'obs_delay'.*whole control steps"):
        sw.delays(12, 2, obs_delay=16)


def test_cli_options():
    base = ["--checkpoint", "x.pth"]
    a = play.parse_args(base)
    assert a.action_delay == 0 and a.obs_delay == 0
    a = play.parse_args(base + ["--action-delay", "2", "--obs-delay", "15"])
    assert (a.action_delay, a.obs_delay) == (2, 15)
    a = play.parse_args(base + ["--sweep", "action_delay=0,1,2,3", "--paired", "--paired-diff", "--baseline", "0", "--obs-delay", "1", "--paired-out", "d.json",
                                "--sweep-out", "c.json"])
    assert play.Sweep.parse(a.sweep, paired=a.paired).cell_delays(a.action_delay, a.obs_delay) == dict(action_delay=[0, 1, 2, 3], obs_delay=[1] * 4)
    for bad in (["--action-delay", "16"], ["--obs-delay", "-1"], ["--action-delay", "1.5"], ["--sweep", "action_delay=0.5,1"], ["--sweep", "obs_delay=0:3:3"]):
        with pytest.raises(SystemExit):
            play.parse_args(base + bad)
    line = play.latency_line(dict(control_dt=0.0125, action_delay=[0, 2], obs_delay=[1, 1]))
    assert line == "latency: control dt 12.5 ms; action_delay 0,2 steps = 0,25 ms; obs_delay 1,1 steps = 12.5,12.5 ms"


# ------------------------------------------------------------------------------------------------------- the shim under sanitizers
def test_shim_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (tests/csrc/play_delay_sanitize_main.cpp: the shim plus a main over one case per width, the ring sized by
    pp_play_delay_ring_bytes' arithmetic), built with -fsanitize=address,undefined and run on its own; never loaded into Python."""
    exe = tmp_path / "play_delay_sanitize"
    src = os.path.join(_HERE, "csrc", "play_delay_sanitize_main.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", str(exe), src],
                   check=True, capture_output=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    assert res.stdout.count("checksum") == 6
