"""Observation and action history, the part that needs no GPU (isaacgym_amd.history; include/ppenv_history.h): the device header's column
map and piece walk compiled for the host against history.reference, bit for bit and at every 4-byte phase of rows and slots; the
reference itself against hand-written cases; parse and its refusals; pp_history_width; and every refusal of pp_history_push, by the field
its message names, before any device call."""
import numpy as np
import pytest
import torch

import history_shim_binding as hs
from isaacgym_amd import _lib, history


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------ the numpy restatement
def test_reference_on_a_hand_written_case():
    n, A, Ho, Ha = 2, 1, 2, 2
    o0 = np.array([[1, 2], [3, 4]], np.float32)
    w0 = history.reference(None, o0, None, None, n, A, Ho, Ha)
    assert w0.tolist() == [[1, 2, 1, 2, 1, 2, 0, 0], [3, 4, 3, 4, 3, 4, 0, 0]]                      # every row starts: first sample held, no actions
    o1 = np.array([[5, 6], [7, 8]], np.float32)
    a0 = np.array([[0.5], [-3.0]], np.float32)
    w1 = history.reference(w0, o1, a0, np.array([0, 0]), n, A, Ho, Ha)
    assert w1.tolist() == [[5, 6, 1, 2, 1, 2, 0.5, 0], [7, 8, 3, 4, 3, 4, -1.0, 0]]                 # the slots move up; a_1 clamped
    o2 = np.array([[9, 10], [11, 12]], np.float32)
    a1 = np.array([[np.nan], [0.25]], np.float32)
    w2 = history.reference(w1, o2, a1, np.array([0, 1 << 32]), n, A, Ho, Ha)
    assert w2.tolist() == [[9, 10, 5, 6, 1, 2, -1.0, 0.5], [11, 12, 11, 12, 11, 12, 0, 0]]          # a NaN action is lo; row 1 reset (64-bit word)
    # two rows per env: agent 0's word alone decides, for both rows
    w3 = history.reference(w2, o1, a0, np.array([0, 7]), n, A, Ho, Ha, num_agents=2)
    assert w3[1].tolist() == [7, 8, 11, 12, 11, 12, -1.0, 0]
    w4 = history.reference(w2, o1, a0, np.array([3, 0]), n, A, Ho, Ha, num_agents=2)
    assert w4.tolist() == [[5, 6, 5, 6, 5, 6, 0, 0], [7, 8, 7, 8, 7, 8, 0, 0]]
    # bit for bit: a NaN payload and a negative zero in an observation survive
    odd = np.array([[0x7FC00123, 0x80000000]], np.uint32).view(np.float32)
    w = history.reference(None, odd, None, None, n, A, 1, 0)
    assert w.view(np.uint32).tolist() == [[0x7FC00123, 0x80000000] * 2]
    # -0.0 in an action keeps its sign through the clamp
    w = history.reference(np.zeros((1, 3), np.float32), np.ones((1, 2), np.float32), np.array([[-0.0]], np.float32), None, 2, 1, 0, 1)
    assert w.view(np.uint32).tolist() == [[0x3F800000, 0x3F800000, 0x80000000]]


# ------------------------------------------------------------------------------------------------------ the column map
@pytest.mark.parametrize("n, A", hs.SHAPES + ((1, 1), (2, 2)), ids=lambda v: str(v))
@pytest.mark.parametrize("Ho, Ha", hs.HISTORIES, ids=lambda v: str(v))
def test_column_map_names_every_word_once_and_its_runs_are_contiguous(n, A, Ho, Ha):
    W = hs.lib().history_shim_width(n, A, Ho, Ha)
    assert W == (Ho + 1) * n + Ha * A == history.width(n, A, Ho, Ha)
    e = (Ho + 1) * n
    for start in (False, True):
        for c in range(W):
            kind, col, left = hs.shim_source(n, A, Ho, Ha, start, c)
            if c < n:
                want = (hs.OBS, c)
            elif c < e:
                want = (hs.OBS, c % n) if start else (hs.PREV, c - n)
            elif start:
                want = (hs.ZERO, 0)
            elif c < e + A:
                want = (hs.ACT, c - e)
            else:
                want = (hs.PREV, c - A)
            assert (kind, col) == want, (start, c)
            assert 1 <= left <= W - c
            for i in range(1, min(left, 5)):                                                   # a run: the same source, consecutive words
                k2, c2, l2 = hs.shim_source(n, A, Ho, Ha, start, c + i)
                assert k2 == kind and l2 == left - i and (kind == hs.ZERO or c2 == col + i)


# ------------------------------------------------------------------------------------------------------ the kernel body on the host
@pytest.mark.parametrize("n, A", hs.SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("Ho, Ha", hs.HISTORIES, ids=lambda v: str(v))
@pytest.mark.parametrize("rows, agents", [(1, 1), (5, 1), (6, 2)])
def test_host_build_of_the_device_header_equals_the_reference_bit_for_bit(n, A, Ho, Ha, rows, agents):
    W = history.width(n, A, Ho, Ha)
    obs, act, dones = hs.case_stream(rows, agents, n, A, pushes=5)
    for pad in (0, 3):                                        # row strides = widths, and widths + 3: row starts at every 4-byte phase
        for phase in range(4):
            band = 5
            bufs = [hs.phased((rows, W + pad + band), (phase + k) % 4, hs.CANARY) for k in range(2)]
            prev_ref = prev = None
            for t in range(obs.shape[0]):
                o = hs.phased((rows, n + pad), (phase + 1) % 4)
                a = hs.phased((rows, A + pad), (phase + 2) % 4)
                o[:, :n], a[:, :A] = obs[t], act[t - 1] if t else 0
                o[:, n:], a[:, A:] = 123.0, 456.0
                out = bufs[t % 2]
                done = None if t == 0 else dones[t - 1]
                hs.shim_push(o[:, :n], a[:, :A] if t else None, done, None if prev is None else prev[:, :W], out[:, :W], agents, n, A, Ho, Ha)
                want = history.reference(prev_ref, obs[t], act[t - 1] if t else None, done, n, A, Ho, Ha, agents)
                assert np.array_equal(bits(out[:, :W]), bits(want)), (pad, phase, t)
                assert (out[:, W:] == hs.CANARY).all()        # nothing beyond W
                prev, prev_ref = out, want


def test_host_build_takes_the_16_byte_path_and_the_element_path():
    """With everything 16-byte aligned and n, A multiples of 4 every whole piece has an aligned source; one word of phase on the source
    sends every piece down the element path.  Both give the reference."""
    n, A, Ho, Ha, rows = 8, 4, 2, 2, 3
    W = history.width(n, A, Ho, Ha)
    rng = np.random.default_rng(0)
    for src_phase in (0, 1):
        prev, out = hs.phased((rows, W), src_phase), hs.phased((rows, W), 0, hs.CANARY)
        o, a = hs.phased((rows, n), src_phase), hs.phased((rows, A), src_phase)
        prev[...], o[...], a[...] = rng.standard_normal(prev.shape), rng.standard_normal(o.shape), 2 * rng.standard_normal(a.shape)
        done = np.array([0, 1, 0], np.int64)
        hs.shim_push(o, a, done, prev, out, 1, n, A, Ho, Ha)
        assert np.array_equal(bits(out), bits(history.reference(prev, o, a, done, n, A, Ho, Ha)))


# ------------------------------------------------------------------------------------------------------ parse
def test_parse_accepts_pairs_dicts_and_text_and_binds_to_a_task():
    assert history.parse(None) is None and history.parse((0, 0)) is None and history.parse("0,0") is None
    assert history.parse((2, 3)) == history.parse([2, 3]) == history.parse("2,3") == history.parse(" 2 : 3 ") == history.parse(dict(obs=2, actions=3)) == \
        dict(obs=2, actions=3)
    rec = history.parse((2, 2), 80, 7)
    assert rec == dict(obs=2, actions=2, num_obs=80, num_actions=7, width=254)
    assert history.parse(rec, 80, 7) == rec and history.parse(rec) == dict(obs=2, actions=2)
    assert history.parse((2, 2), 313, 27)["width"] == 993
    assert history.parse((0, 1), 80, 7)["width"] == 87 and history.parse((1, 0), 80, 7)["width"] == 160
    assert history.text(rec) == "history: 2 observations + 2 actions back: first layer K 80 -> 254 (padded 256)"


@pytest.mark.parametrize("bad", [(9, 0), (0, 9), (-1, 2), (1.5, 0), (True, 1), (1,), (1, 2, 3), "1", "a,b", "1,2,3", 5, dict(obs=1), dict(obs=1, actions=1, x=2),
                                 (None, 1)], ids=repr)
def test_parse_refuses_by_name(bad):
    with pytest.raises(ValueError, match="history: a history is"):
        history.parse(bad)


def test_bind_and_check_record_refuse_by_name():
    with pytest.raises(ValueError, match="wider than 16256"):
        history.parse((8, 8), 2000, 27)
    with pytest.raises(ValueError, match="num_obs = 80, here num_obs = 313"):
        history.parse(history.parse((2, 2), 80, 7), 313, 7)
    a, b = history.parse((2, 2), 80, 7), history.parse((2, 1), 80, 7)
    history.check_record(a, dict(a))
    history.check_record(None, None)
    with pytest.raises(ValueError, match=r"trained with history \{'obs': 2, 'actions': 2.*this trainer has history \{'obs': 2, 'actions': 1"):
        history.check_record(a, b)
    with pytest.raises(ValueError, match="trained with no history, this trainer has history"):
        history.check_record(None, a)
    with pytest.raises(ValueError, match="this trainer has no history"):
        history.check_record(a, None)


def test_record_round_trips_through_torch_save(tmp_path):
    rec = history.parse((2, 2), 80, 7)
    torch.save({"history": rec}, tmp_path / "ck.pth")
    assert torch.load(tmp_path / "ck.pth", weights_only=True)["history"] == rec


# ------------------------------------------------------------------------------------------------------ the C entry points
def test_width_entry_point():
    L = _lib.lib()
    assert _lib.HISTORY_MAX == 8 and _lib.HISTORY_MAX_WIDTH == 16256
    assert L.pp_history_width(80, 7, 2, 2) == 254 and L.pp_history_width(313, 27, 2, 2) == 993 and L.pp_history_width(313, 27, 8, 8) == 3033
    assert L.pp_history_width(80, 7, 1, 0) == 160 and L.pp_history_width(80, 7, 0, 1) == 87
    assert L.pp_history_width(1806, 1, 8, 2) == 16256 and L.pp_history_width(1806, 1, 8, 3) == 0      # the limit itself, and one word more
    for bad in ((0, 7, 1, 1), (80, 0, 1, 1), (80, 7, 0, 0), (80, 7, 9, 0), (80, 7, 0, 9), (80, 7, -1, 1), (80, 7, 1, -1), (2 ** 31 - 1, 7, 8, 8)):
        assert L.pp_history_width(*bad) == 0, bad
    for n, A in hs.SHAPES:
        for Ho, Ha in hs.HISTORIES:
            assert L.pp_history_width(n, A, Ho, Ha) == history.width(n, A, Ho, Ha) == hs.lib().history_shim_width(n, A, Ho, Ha)


def test_push_refuses_bad_arguments_before_any_device_call_naming_the_field():
    L = _lib.lib()
    err = lambda: L.ppenv_last_error().decode()
    ok = dict(obs=4096, ld_obs=80, act=8192, ld_act=7, done=None, prev=12288, ld_prev=254, next=16384, ld_next=254, rows=4, num_agents=2, n=80, A=7, Ho=2, Ha=2,
              lo=-1.0, hi=1.0, stream=None)
    cases = [(dict(obs=None), "obs is NULL"), (dict(next=None), "next is NULL"), (dict(rows=0), "rows 0 < 1"), (dict(rows=3), "rows 3 < 1 or no multiple of num_agents 2"),
             (dict(num_agents=3), "num_agents 3 is not 1 or 2"), (dict(num_agents=0), "num_agents 0 is not 1 or 2"), (dict(Ho=9), "Ho 9 outside 0..8"),
             (dict(Ho=-1), "Ho -1 outside 0..8"), (dict(Ha=9), "Ha 9 outside 0..8"), (dict(Ha=-1), "Ha -1 outside 0..8"), (dict(Ho=0, Ha=0), "Ho and Ha are both 0"),
             (dict(n=0), "n 0 < 1"), (dict(A=0), "A 0 < 1"), (dict(ld_obs=79), "ld_obs 79 < n 80"), (dict(ld_act=6), "ld_act 6 < A 7"),
             (dict(ld_prev=253), "ld_prev 253 < W 254"), (dict(ld_next=253), "ld_next 253 < W 254"),
             (dict(n=1806, A=1, Ho=8, Ha=3, ld_obs=1806, ld_prev=20000, ld_next=20000), "W 16257 > 16256"), (dict(lo=1.0, hi=-1.0), "lo 1 > hi -1"),
             (dict(prev=16384), "next == prev"), (dict(act=None), "act is NULL with a prev and Ha 2 > 0")]
    for bad, text in cases:
        assert L.pp_history_push(*{**ok, **bad}.values()) == -1, bad
        assert err().startswith("pp_history_push: ") and text in err(), (bad, err())
