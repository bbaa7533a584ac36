"""The training delay line on the MI355X (include/ppenv_train_delay.h; isaacgym_amd.latency.DelayLine).

The kernel against its host build (tests/csrc/train_delay_shim.cpp) byte for byte — outputs with their padding, ages, episode counts,
delays and the whole ring; with lo == hi against play's kernel under a constant table; a captured push replayed; the ABI's refusals.
Need a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import train_delay_shim_binding as td
from test_play_gpu import torch_cuda        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((1, 1), (2, 2), (63, 1), (257, 1), (1025, 1))       # (rows, A)
WIDTHS = (1, 7, 27, 313)                                      # rows per workgroup: 256, 146, 37, 3 -> 1025 rows: 5, 8, 28, 342 workgroups, the last ragged
PUSHES = 40
EINVAL = -1


def words(torch, x):
    """uint32 numpy [.., W] -> the float32 device tensor with those bits."""
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(DEV).view(torch.float32)


def bits(torch, t):
    """A float32 tensor's words as int32 numpy."""
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"rows{s[0]}-A{s[1]}")
def test_kernel_equals_the_shim_byte_for_byte(torch_cuda, shape):
    """An input stride of W + 1, an output stride of W + 3, 40 pushes with random done; a ragged last workgroup, more than one workgroup,
    one row per workgroup up to 256, and row boundaries mid-wave (W = 7, 27)."""
    torch = torch_cuda
    from isaacgym_amd import scene
    from isaacgym_amd.latency import DelayLine
    rows, A = shape
    seed = scene.stream_seed(42, scene.STREAM_LATENCY)
    for W in WIDTHS:
        xs, dones = td.case_stream(rows, A, W, PUSHES, pad=1, p_done=0.15)
        x_dev, done_dev = words(torch, xs), torch.from_numpy(dones).to(DEV)
        keep = x_dev.clone()
        for k, (lo, hi) in enumerate(td.RANGES):
            channel, offset = k % 2, 1000 * k
            h = td.HostLine(rows, W, lo, hi, A, seed, offset, channel, ld_out=W + 3)
            dl = DelayLine(rows, W, lo, hi, DEV, num_agents=A, seed=seed, env_id_offset=offset, channel=channel)
            out = torch.zeros((PUSHES, rows, W + 3), dtype=torch.float32, device=DEV)
            state = []
            for t in range(PUSHES):
                dl.push(x_dev[t][:, :W], None if t == 0 else done_dev[t], out[t][:, :W])
                state.append(torch.stack([dl.age, dl.episode, dl.delays]))
            got, state = bits(torch, out), torch.stack(state).cpu().numpy()
            for t in range(PUSHES):
                h.push(xs[t], None if t == 0 else dones[t])
                where = (rows, A, W, lo, hi, t)
                assert np.array_equal(got[t], h.out.view(np.int32)), where                     # the data and the untouched padding
                assert np.array_equal(state[t], np.stack([h.age, h.episode, h.delay])), where
            assert np.array_equal(bits(torch, dl.ring), h.ring.view(np.int32)), (rows, A, W, lo, hi)
            assert h.delay.min() >= lo and h.delay.max() <= hi
        assert torch.equal(x_dev.view(torch.int32), keep.view(torch.int32))                    # the input, its padding included, is not modified


@pytest.mark.parametrize("d", (0, 1, 3, 15))
def test_a_fixed_delay_is_plays_kernel_with_a_constant_table(torch_cuda, d):
    """lo == hi: out, age and the ring equal pp_play_delay_push under delays = d, byte for byte."""
    torch = torch_cuda
    from isaacgym_amd.latency import DelayLine
    from isaacgym_amd.play import Delay
    for rows, A, W in ((130, 2, 27), (257, 1, 7), (65, 1, 313)):
        xs, dones = td.case_stream(rows, A, W, PUSHES, pad=0, p_done=0.15)
        x_dev, done_dev = words(torch, xs), torch.from_numpy(dones).to(DEV)
        new, old = DelayLine(rows, W, d, d, DEV, num_agents=A, seed=7), Delay(rows, W, np.full(rows, d, np.int32), DEV, num_agents=A)
        out = torch.zeros((rows, W), dtype=torch.float32, device=DEV)
        for t in range(PUSHES):
            done = None if t == 0 else done_dev[t]
            new.push(x_dev[t], done, out)
            want = old.push(x_dev[t], done)
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (rows, W, t)
            assert torch.equal(new.age, old.age), (rows, W, t)
        assert torch.equal(new.ring.view(torch.int32), old.ring.view(torch.int32)) and (new.delays == d).all()


def test_a_captured_push_replays_like_eager_pushes(torch_cuda):
    """No host-side counter, the draw included: one captured push replayed 40 times equals 40 eager pushes."""
    torch = torch_cuda
    from isaacgym_amd.latency import DelayLine
    rows, A, W = 130, 2, 27
    xs, dones = td.case_stream(rows, A, W, PUSHES, pad=0, p_done=0.15)
    x_dev, done_dev = words(torch, xs), torch.from_numpy(dones).to(DEV)
    eager, replayed = (DelayLine(rows, W, 0, 3, DEV, num_agents=A, seed=11, env_id_offset=5, channel=1) for _ in range(2))
    out_e, out_r = (torch.zeros((rows, W), dtype=torch.float32, device=DEV) for _ in range(2))
    want = [(eager.push(x_dev[t], done_dev[t], out_e).clone(), eager.delays.clone()) for t in range(PUSHES)]
    x, done = x_dev[0].clone(), done_dev[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        replayed.push(x, done, out_r)                                                       # warm-up outside the capture ...
        replayed.reset()                                                                    # ... undone
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.push(x, done, out_r)
    replayed.reset()                                                                        # the capture itself ran nothing
    for t in range(PUSHES):
        x.copy_(x_dev[t])
        done.copy_(done_dev[t])
        graph.replay()
        assert torch.equal(out_r.view(torch.int32), want[t][0].view(torch.int32)) and torch.equal(replayed.delays, want[t][1]), t
    assert torch.equal(replayed.age, eager.age) and torch.equal(replayed.episode, eager.episode)


def test_the_abi_refuses_before_any_launch(torch_cuda):
    """Everything pp_play_delay_push refuses, and lo < 0, lo > hi, hi > 15, a channel that is not 0 or 1: PPENV_EINVAL with its message, and
    no word of the state or the output changes."""
    torch = torch_cuda
    from isaacgym_amd import _lib
    L = _lib.lib()
    rows, A, W = 8, 2, 5
    x = torch.ones((rows, W), device=DEV)
    done = torch.ones(rows, dtype=torch.int64, device=DEV)
    delay, age, episode = (torch.full((rows,), 77, dtype=torch.int32, device=DEV) for _ in range(3))
    ring = torch.full((16, rows, W), 5.0, device=DEV)
    out = torch.full((rows, W), 9.0, device=DEV)
    st = _lib.stream(x)

    def push(lo=0, hi=3, channel=0, consts=True, **kw):
        a = dict(x=x.data_ptr(), ld_in=W, done=done.data_ptr(), rows=rows, A=A, W=W, delay=delay.data_ptr(), age=age.data_ptr(), episode=episode.data_ptr(),
                 ring=ring.data_ptr(), out=out.data_ptr(), ld_out=W)
        a.update(kw)
        c = _lib.TrainDelayConsts(lo, hi, 1, 0, channel)
        rc = L.pp_train_delay_push(a["x"], a["ld_in"], a["done"], a["rows"], a["A"], a["W"], C.byref(c) if consts else None, a["delay"], a["age"], a["episode"],
                                   a["ring"], a["out"], a["ld_out"], st)
        return rc, L.ppenv_last_error().decode()

    cases = [(dict(lo=-1), "lo -1 < 0"), (dict(lo=3, hi=2), "lo 3 > hi 2"), (dict(hi=16), "hi 16 > 15"), (dict(channel=2), "channel 2"), (dict(channel=-1), "channel -1"),
             (dict(consts=False), "NULL constants")]
    cases += [(kw, "NULL pointer (done excepted)") for kw in (dict(x=None), dict(delay=None), dict(age=None), dict(episode=None), dict(ring=None), dict(out=None),
                                                              dict(rows=0), dict(rows=7), dict(A=0), dict(A=3), dict(W=0), dict(W=513), dict(ld_in=W - 1),
                                                              dict(ld_out=W - 1))]
    for kw, text in cases:
        rc, msg = push(**kw)
        assert rc == EINVAL and msg.startswith("pp_train_delay_push: ") and text in msg, (kw, rc, msg)
    assert L.pp_train_delay_reset(0, age.data_ptr(), episode.data_ptr(), st) == EINVAL and "pp_train_delay_reset" in L.ppenv_last_error().decode()
    assert L.pp_train_delay_reset(rows, None, episode.data_ptr(), st) == EINVAL and L.pp_train_delay_reset(rows, age.data_ptr(), None, st) == EINVAL
    assert (delay == 77).all() and (age == 77).all() and (episode == 77).all() and (ring == 5.0).all() and (out == 9.0).all()
    assert L.pp_train_delay_ring_bytes(rows, W, 3) == 4 * 4 * rows * W and L.pp_train_delay_table_bytes(rows) == 4 * rows
    assert L.pp_train_delay_ring_bytes(rows, W, 16) == 0 and L.pp_train_delay_ring_bytes(rows, W, -1) == 0 and L.pp_train_delay_ring_bytes(0, W, 3) == 0
    assert L.pp_train_delay_table_bytes(0) == 0
    rc, msg = push(done=None)                                                               # done may be NULL: accepted, and it runs
    assert rc == 0
    assert (age == 78).all() and (episode == 77).all()                                      # age 77: no episode starts


def test_delay_line_checks_its_arguments_on_the_host(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.latency import DelayLine
    for kw in (dict(rows=0), dict(rows=3, num_agents=2), dict(num_agents=3), dict(width=0), dict(width=513), dict(lo=-1), dict(lo=2, hi=1), dict(hi=16),
               dict(channel=2), dict(env_id_offset=-1)):
        a = dict(rows=4, width=3, lo=0, hi=2, device=DEV, num_agents=1, seed=1, env_id_offset=0, channel=0)
        a.update(kw)
        with pytest.raises(ValueError, match="DelayLine"):
            DelayLine(**a)
    dl = DelayLine(4, 3, 0, 2, DEV)
    good, out = torch.zeros((4, 3), device=DEV), torch.zeros((4, 3), device=DEV)
    for bad in (torch.zeros((3, 4), device=DEV).t(), good.double(), good[:-1], good.cpu()):
        with pytest.raises(ValueError, match="DelayLine.push: x"):
            dl.push(bad, None, out)
        with pytest.raises(ValueError, match="DelayLine.push: out"):
            dl.push(good, None, bad)
    with pytest.raises(ValueError, match="DelayLine.push: done"):
        dl.push(good, torch.zeros(4, dtype=torch.int32, device=DEV), out)
    assert not dl.age.any()                                                                 # nothing was launched
