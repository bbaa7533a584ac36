"""The observation and action history kernel on the MI355X (pp_history_push; include/ppenv_history.h) against history.reference, bit for
bit on int32 views: six chained pushes from no previous row under scripted dones (both agent words of a 2-agent env, a done of 2^32), at
row counts around the workgroup's row tile, both tasks' (n, A), four histories, row strides equal to the widths and three words wider —
row starts at every 4-byte phase — with NaNs, negative zeros and actions beyond [-1, 1] in the inputs, a canary beyond W, and the same
sequence captured in a graph and replayed.  Need a real MI355X."""
import numpy as np
import pytest

import history_shim_binding as hs
from test_play_gpu import torch_cuda        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 6


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def chain(history, obs, act, dones, agents, n, A, Ho, Ha):
    """The reference applied T times from no previous row -> [T, rows, W]."""
    out, prev = [], None
    for t in range(obs.shape[0]):
        prev = history.reference(prev, obs[t], act[t - 1] if t else None, dones[t - 1] if t else None, n, A, Ho, Ha, agents)
        out.append(prev)
    return np.stack(out)


@pytest.mark.parametrize("n, A", hs.SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("rows, agents", [(1, 1), (63, 1), (64, 1), (65, 1), (130, 1), (64, 2), (130, 2)])
def test_chained_pushes_equal_the_reference_bit_for_bit_eager_and_replayed(torch_cuda, rows, agents, n, A):
    torch = torch_cuda
    from isaacgym_amd import history
    obs, act, dones = hs.case_stream(rows, agents, n, A, pushes=T)
    assert (dones == 1 << 32).any() and (agents == 1 or (dones[:, 1::2] != dones[:, 0::2]).any())
    assert np.isnan(obs).any() and np.isnan(act).any() and (np.abs(act) > 1).any() and np.signbit(obs[obs == 0]).any()
    d_d = torch.from_numpy(dones).to(DEV)
    for Ho, Ha in hs.HISTORIES:
        W = history.width(n, A, Ho, Ha)
        want = chain(history, obs, act, dones, agents, n, A, Ho, Ha)
        stack = history.HistoryStack(rows, n, A, Ho, Ha, DEV, agents)
        assert stack.width == W and stack.record() == history.parse((Ho, Ha), n, A)
        for pad in (0, 3):                                     # every stride equal to its width; and width + 3
            o_h, a_h = np.full((T, rows, n + pad), 123.0, np.float32), np.full((T, rows, A + pad), 456.0, np.float32)
            o_h[:, :, :n], a_h[:, :, :A] = obs, act
            o_d, a_d = torch.from_numpy(o_h).to(DEV), torch.from_numpy(a_h).to(DEV)

            def run(out):
                for t in range(T):
                    stack.push(o_d[t][:, :n], a_d[t - 1][:, :A] if t else None, d_d[t - 1] if t else None, out[t - 1][:, :W] if t else None, out[t][:, :W])

            # one slab more than is written: with pad 0 the canary is the slab after the last row, with pad 3 also every row's last 3 words
            eager = torch.full((T + 1, rows, W + pad), float(hs.CANARY), dtype=torch.float32, device=DEV)
            run(eager)
            torch.cuda.synchronize()
            got = eager.cpu().numpy()
            assert np.array_equal(bits(got[:T, :, :W]), bits(want)), (Ho, Ha, pad)
            assert (got[:T, :, W:] == hs.CANARY).all() and (got[T] == hs.CANARY).all(), (Ho, Ha, pad)
            replayed = torch.full_like(eager, float(hs.CANARY))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(replayed)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32)), (Ho, Ha, pad)


def test_advance_alternates_two_buffers_and_reset_starts_every_row(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import history
    rows, agents, n, A, Ho, Ha = 6, 2, 80, 7, 2, 2
    obs, act, dones = hs.case_stream(rows, agents, n, A, pushes=4)
    want = chain(history, obs, act, dones, agents, n, A, Ho, Ha)
    stack = history.HistoryStack(rows, n, A, Ho, Ha, DEV, agents)
    o_d, a_d, d_d = (torch.from_numpy(x).to(DEV) for x in (obs, act, dones))
    for again in range(2):
        seen = []
        for t in range(4):
            wide = stack.advance(o_d[t], a_d[t - 1] if t else None, d_d[t - 1] if t else None)
            seen.append(wide.data_ptr())
            assert np.array_equal(bits(wide.cpu().numpy()), bits(want[t])), (again, t)
        assert seen[0] == seen[2] != seen[1] == seen[3]
        stack.reset()
    with pytest.raises(ValueError, match="HistoryStack.push: obs must be float32"):
        stack.advance(o_d[0][:, :n - 1], None, None)
    with pytest.raises(ValueError, match="HistoryStack: rows 5"):
        history.HistoryStack(5, n, A, Ho, Ha, DEV, 2)
