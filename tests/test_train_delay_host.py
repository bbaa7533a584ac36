"""The training delay line's rule and draw, on the CPU (include/ppenv_train_delay.h; isaacgym_amd.latency; scene.latency_draws).

The rule is this build's own specification — the reference delays nothing — so it is pinned by restating it twice: a g++ build of the
device header the kernel compiles (tests/csrc/train_delay_shim.cpp) and numpy (train_delay_shim_binding.NumpyLine, which redraws at each
episode start with scene.latency_draws).  The shim also runs under the address and undefined-behaviour sanitizers as a stand-alone
program.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import train_delay_shim_binding as td
from isaacgym_amd import _lib, latency, scene

SEEDS = (0, 42, 43, 12345)
SPANS = (1, 2, 4, 16)
GIDS, EPISODES = np.arange(4096).reshape(-1, 1), np.arange(16).reshape(1, -1)


@pytest.fixture(scope="module")
def tables():
    """{(user seed, span, channel): the shim's draws [4096, 16]} with lo = 1 (lo + span - 1 <= 15 only for span < 16: lo = 0 there)."""
    out = {}
    for s in SEEDS:
        for span in SPANS:
            lo = 0 if span == 16 else 1
            for ch in (0, 1):
                out[s, span, ch] = td.shim_draws(scene.stream_seed(s, scene.STREAM_LATENCY), GIDS, EPISODES, ch, lo, lo + span - 1)
    return out


def test_the_stream_salt_is_the_next_words_of_the_constant():
    """The salts are consecutive 64-bit words of the hexadecimal expansion of pi's fraction; STREAM_LATENCY follows STREAM_SERVES."""
    assert scene.STREAM_LATENCY == 0x452821E638D01377
    assert len({scene.STREAM_ENV, scene.STREAM_TABLES, scene.STREAM_SAMPLER, scene.STREAM_SERVES, scene.STREAM_LATENCY}) == 5


def test_draws_of_the_shim_equal_latency_draws_exactly(tables):
    for (s, span, ch), got in tables.items():
        lo = 0 if span == 16 else 1
        want = scene.latency_draws(scene.stream_seed(s, scene.STREAM_LATENCY), GIDS, EPISODES, ch, lo, lo + span - 1)
        assert want.dtype == np.int32 and want.shape == (4096, 16)
        assert np.array_equal(got, want), (s, span, ch)
        assert got.min() >= lo and got.max() <= lo + span - 1, (s, span, ch)
        if span == 1:
            assert (got == lo).all()
        else:
            assert got.min() == lo and got.max() == lo + span - 1, (s, span, ch)             # both ends are drawn


def test_draws_are_uniform(tables):
    """Every value's count over the 65 536 keys within 5 sigma of n / S (binomial).  A condition on a fixed function: checked on the CPU for
    this hash and salt, the worst case is 2.8 sigma."""
    n = GIDS.size * EPISODES.size
    assert n == 65536
    worst = 0.0
    for (s, span, ch), got in tables.items():
        if span == 1:
            continue
        counts = np.bincount(got.ravel() - got.min(), minlength=span)
        sigma = np.sqrt(n * (1.0 / span) * (1.0 - 1.0 / span))
        dev = np.abs(counts - n / span).max() / sigma
        worst = max(worst, dev)
        assert dev <= 5.0, (s, span, ch, counts.tolist())
    print(f"worst deviation {worst:.2f} sigma")


def test_draws_differ_across_channels_and_seeds(tables):
    for span in (2, 4, 16):
        for s in SEEDS:
            assert not np.array_equal(tables[s, span, 0], tables[s, span, 1]), (s, span)
        for ch in (0, 1):
            assert not np.array_equal(tables[42, span, ch], tables[43, span, ch]), (span, ch)
            # unrelated, not merely different: about 1 / span of the keys agree
            agree = (tables[42, span, ch] == tables[43, span, ch]).mean()
            assert abs(agree - 1.0 / span) < 0.02, (span, ch, agree)


def test_latency_draws_refuses_what_the_kernel_refuses():
    for lo, hi, ch in ((-1, 2, 0), (3, 2, 0), (0, 16, 0), (0, 3, 2), (0, 3, -1)):
        with pytest.raises(ValueError):
            scene.latency_draws(1, [0], [0], ch, lo, hi)
    assert scene.latency_draws(1, 7, 3, 1, 5, 5).tolist() == [5]                              # scalars broadcast to one draw


@pytest.mark.parametrize("rng", td.RANGES, ids=lambda r: f"{r[0]}-{r[1]}")
@pytest.mark.parametrize("channel", (0, 1))
def test_the_rule_against_numpy(rng, channel):
    """60 pushes, done on about 10 % of the env-steps, rows 6 with A = 2, width 5: out, age, episode, delay and the whole ring, bitwise."""
    rows, A, W, T = 6, 2, 5, 60
    lo, hi = rng
    seed = scene.stream_seed(42, scene.STREAM_LATENCY)
    xs, dones = td.case_stream(rows, A, W, T, pad=1)
    assert 0.03 < (dones[:, ::A] != 0).mean() < 0.2
    h, ref = td.HostLine(rows, W, lo, hi, A, seed, 100, channel), td.NumpyLine(rows, W, lo, hi, A, seed, 100, channel)
    seen = set()
    for t in range(T):
        done = None if t == 0 else dones[t]
        got, want = h.push(xs[t], done), ref.push(xs[t], done)
        assert np.array_equal(got, want), t
        assert np.array_equal(h.age, ref.age) and np.array_equal(h.episode, ref.episode) and np.array_equal(h.delay, ref.delay), t
        assert np.array_equal(h.ring, ref.ring), t
        assert np.array_equal(h.delay[0::2], h.delay[1::2])                                   # both rows of an env hold the env's delay
        assert h.delay.min() >= lo and h.delay.max() <= hi
        seen |= set(h.delay.tolist())
    assert h.episode.min() >= 2                                                             # every row restarted
    assert len(seen) > 1 or lo == hi or hi == 0
    h.reset()
    assert not h.age.any() and not h.episode.any()


def test_a_fixed_delay_is_exactly_that_old():
    """lo == hi == 3, no done: from push 3 on every output is the input of 3 pushes ago; before, the first sample."""
    rows, W = 4, 3
    xs, _ = td.case_stream(rows, 1, W, 10, pad=0)
    h = td.HostLine(rows, W, 3, 3)
    for t in range(10):
        assert np.array_equal(h.push(xs[t]), xs[max(t - 3, 0)]), t


def test_the_ctypes_mirror_matches_the_header():
    """_lib.TrainDelayConsts against the struct in include/ppenv_train_delay.h (field order and types) and the shim binding's own mirror."""
    text = open(os.path.join(_lib.ROOT, "include", "ppenv_train_delay.h")).read()
    body = re.search(r"typedef struct pp_train_delay_consts \{(.*?)\} pp_train_delay_consts;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|uint64_t)\s+([\w\s,]+);", body):
        fields += [(n.strip(), {"int32_t": C.c_int32, "uint64_t": C.c_uint64}[ctype]) for n in names.split(",")]
    assert fields == list(_lib.TrainDelayConsts._fields_) == list(td.Consts._fields_)
    assert C.sizeof(_lib.TrainDelayConsts) == 24 and _lib.TrainDelayConsts.seed.offset == 8


def test_the_entries_are_declared_and_bound():
    text = open(os.path.join(_lib.ROOT, "include", "ppenv_train_delay.h")).read()
    names = re.findall(r"^(?:int|size_t)\s+(pp_train_delay_\w+)\(", text, re.M)
    assert sorted(names) == ["pp_train_delay_push", "pp_train_delay_reset", "pp_train_delay_ring_bytes", "pp_train_delay_table_bytes"]
    src = open(os.path.join(_lib.ROOT, "isaacgym_amd", "_lib.py")).read()
    for n in names:
        assert f"L.{n}.argtypes" in src, n
    assert any(p.endswith("ppenv_train_delay.hip") for p in _lib.SOURCES)


def test_shim_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (tests/csrc/train_delay_sanitize_main.cpp: the shim plus a main over one case per width, the ring sized by
    pp_train_delay_ring_bytes' arithmetic, the tables starting as garbage), built with -fsanitize=address,undefined and run on its own;
    never loaded into Python."""
    exe = tmp_path / "train_delay_sanitize"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "train_delay_sanitize_main.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", str(exe), src],
                   check=True, capture_output=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    assert res.stdout.count("checksum") == 6


# ---------------------------------------------------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("value, want", [(0, (0, 0)), (3, (3, 3)), (15, (15, 15)), ((0, 2), (0, 2)), ([1, 1], (1, 1)), ("2", (2, 2)), ("0:3", (0, 3)),
                                          ("15:15", (15, 15)), (2.0, (2, 2)), (np.int64(4), (4, 4)), ((np.int32(1), 3), (1, 3))])
def test_a_delay_argument_parses(value, want):
    assert latency.delay_range("--action-delay", value) == want


@pytest.mark.parametrize("value", [-1, 16, (2, 1), (0, 16), (-1, 2), 1.5, "1.5", "a", "", "1:2:3", "3:1", "-1", "0:16", ":", "1:", (1,), (1, 2, 3), None, True,
                                   (0.5, 2), "1e0"])
def test_a_malformed_delay_argument_names_itself(value):
    with pytest.raises(ValueError, match="--obs-delay"):
        latency.delay_range("--obs-delay", value)


def test_the_cli_refuses_a_malformed_delay_before_anything_is_built():
    from isaacgym_amd import ppo
    for argv in (["--action-delay", "3:1"], ["--obs-delay", "16"], ["--action-delay", "x"]):
        with pytest.raises(ValueError, match=argv[0]):
            ppo.main(argv)


def test_the_start_up_line_names_steps_and_milliseconds():
    line = latency.latency_text(dict(control_dt=1.0 / 60.0, action_delay=[0, 3], obs_delay=[1, 1]))
    assert line == "latency: control dt 16.6667 ms; action_delay 0..3 steps = 0..50 ms, drawn per episode; obs_delay 1 steps = 16.6667 ms"
