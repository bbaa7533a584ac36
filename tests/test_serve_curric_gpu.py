"""The serve curriculum's four launches on the MI355X (include/ppenv_serve_curric.h) against the host build of the same per-env and per-bin
code (serve_curric_shim_binding.HostCurric), bit for bit, on the same streams of rewards and dones: a partial last workgroup, 1 / 3 / 256
bins, horizons of 1 and 8 steps, both layouts, one and two rows per env, the step where every env finishes and the one where none does, a
fold over more than one chunk, and a captured step replayed.  Need a real MI355X."""
import numpy as np
import pytest

import serve_curric_shim_binding as scb
from isaacgym_amd import _lib, scene, serve
from test_play_gpu import torch_cuda        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SOA, AOS = _lib.SERVE_LAYOUT_SOA3, _lib.SERVE_LAYOUT_AOS5
SEED = scene.stream_seed(9, scene.STREAM_SERVES)
OFFSET = 17


class Handle:
    """What curriculum.ServeCurriculum asks of an env handle, without an env: the library, the sizes and the override buffer."""

    def __init__(self, torch, n, layout, A):
        self.L, self.device, self.num_envs, self.num_agents = _lib.lib(), torch.device(DEV), n, A
        self.form = scene.VARIANT_TN if layout == AOS else (scene.VARIANT_T4 if A == 2 else scene.VARIANT_TT)
        self.layout = layout
        self.out = torch.zeros((3, n), dtype=torch.float32, device=DEV) if layout == SOA else None

    def serve_defaults(self):
        return scb.DEFAULTS

    def serve_target(self):
        return dict(axes=serve.AXES_27DOF, out=self.out, form=self.form, layout=self.layout, reset_rows=self.num_agents, seed=SEED, env_id_offset=OFFSET)


def make(torch, n, B, H, layout, A, **kw):
    from isaacgym_amd.curriculum import ServeCurriculum
    env = Handle(torch, n, layout, A)
    dev = ServeCurriculum(env, scb.grid_bins(B), horizon=H, **kw)
    host = scb.HostCurric(n, scb.grid_bins(B), env.form, layout, reset_rows=A, num_agents=A, seed=SEED, env_id_offset=OFFSET, **kw)
    return dev, host


def dev_words(torch, dev):
    """The device state as serve_curric_shim_binding's words() gives the host's."""
    out = {}
    for k in scb.HostCurric.NAMES + ("out",):
        t = getattr(dev, k).contiguous()
        out[k] = t.cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint64)
    return out


CASES = [(1, 1, 1, SOA, 1), (1, 3, 8, AOS, 1), (257, 3, 8, SOA, 1), (257, 256, 1, SOA, 2), (257, 3, 8, AOS, 2), (1000, 256, 8, SOA, 1), (1000, 3, 8, SOA, 2),
         (1000, 1, 8, AOS, 1), (1000, 256, 8, AOS, 1)]


@pytest.mark.parametrize("n, B, H, layout, A", CASES, ids=[f"n{n}-b{B}-h{H}-{'soa3' if lay == SOA else 'aos5'}-a{A}" for n, B, H, lay, A in CASES])
def test_four_launches_match_the_host_build(torch_cuda, n, B, H, layout, A):
    torch = torch_cuda
    dev, host = make(torch, n, B, H, layout, A, power=2, mix=0.1, alpha=0.3)
    assert not scb.same_words(dev_words(torch, dev), host.words())                             # fill
    steps = 24 if H == 8 else 16
    rew, reset = scb.scripted(steps, n, A, A)
    d_rew, d_reset = torch.from_numpy(rew).to(DEV), torch.from_numpy(reset).to(DEV)
    fin_bin, fin_q = np.full((H, n), -1, np.int32), np.zeros((H, n), np.int64)
    games = 0
    for t in range(steps):
        r = t % H
        dev.step(r, d_rew[t], d_reset[t])
        host.step(rew[t], reset[t], fin_bin[r], fin_q[r])
        assert not scb.same_words(dev_words(torch, dev), host.words()), (t, scb.same_words(dev_words(torch, dev), host.words()))
        assert np.array_equal(dev.fin_bin[r].cpu().numpy(), fin_bin[r]), t
        live = fin_bin[r] >= 0
        assert np.array_equal(dev.fin_q[r].cpu().numpy()[live], fin_q[r][live]), t
        fired = reset[t][::A] != 0
        if t == 6:
            assert fired.all()                                                                 # every env finishes in this step
        if t == 7:
            assert not fired.any() and (fin_bin[r] == -1).all()                                # ... and none in this one
        if r == H - 1:
            tot = host.fold(fin_bin, fin_q)
            assert np.array_equal(dev.fold().cpu().numpy(), tot), t
            games += int(tot[0].sum())
            dev.update()
            host.update(tot)
            assert not scb.same_words(dev_words(torch, dev), host.words()), (t, "update")
    assert games > 0 and int(host.games.sum()) == games
    table = dev.table()
    assert np.array_equal(table["prob"].cpu().numpy(), host.prob()) and abs(float(table["prob"].sum()) - 1.0) < 1e-12
    if n >= 4:
        assert int(host.dropped.sum()) >= 1


def test_every_env_finishing_in_one_bin(torch_cuda):
    """One bin: every finished game is the same bin's, from all workgroups of the step and all lanes of the fold at once."""
    torch = torch_cuda
    n, H = 1000, 8
    dev, host = make(torch, n, 1, H, SOA, 1)
    fin_bin, fin_q = np.full((H, n), -1, np.int32), np.zeros((H, n), np.int64)
    rng = np.random.default_rng(2)
    for t in range(H):
        rew = rng.normal(0, 2, n).astype(np.float32)
        reset = np.full(n, 1 << 32 if t % 2 else 1, np.int64) if t in (2, 5) else np.zeros(n, np.int64)
        dev.step(t, torch.from_numpy(rew).to(DEV), torch.from_numpy(reset).to(DEV))
        host.step(rew, reset, fin_bin[t], fin_q[t])
    tot = host.fold(fin_bin, fin_q)
    assert tot[0, 0] == n and np.array_equal(dev.fold().cpu().numpy(), tot)                    # step 2 ends the uncounted games, step 5 n counted ones
    dev.update()
    host.update(tot)
    assert not scb.same_words(dev_words(torch, dev), host.words())
    assert int(dev.cdf[0]) == 1 << 24


def test_fold_over_more_than_one_chunk(torch_cuda):
    """H * N beyond PP_CURRIC_FOLD_CHUNK and no multiple of it: per-workgroup rows, added in workgroup order by the launch's tail."""
    torch = torch_cuda
    H, n, B = 8, 2 * scb.CHUNK // 8 + 155, 256
    assert (H * n) % scb.CHUNK and H * n > 2 * scb.CHUNK
    dev, host = make(torch, n, B, H, SOA, 1)
    rng = np.random.default_rng(3)
    fin_bin = rng.integers(-1, B, (H, n)).astype(np.int32)
    fin_q = rng.integers(-2 ** 47, 2 ** 47, (H, n)).astype(np.int64)
    fin_q[rng.random((H, n)) < 0.01] = scb.DROPPED
    dev.fin_bin.copy_(torch.from_numpy(fin_bin))
    dev.fin_q.copy_(torch.from_numpy(fin_q))
    want = host.fold(fin_bin, fin_q)
    assert np.array_equal(dev.fold().cpu().numpy(), want) and want[2].sum() > 0
    assert np.array_equal(dev.fold().cpu().numpy(), want)                                      # the workspace is overwritten, not added to
    fin_bin[:] = -1
    dev.fin_bin.fill_(-1)
    assert not dev.fold().any()


def test_captured_step_replays_like_eager(torch_cuda):
    """One captured step launch replayed three times equals three eager launches: the state lives in device memory and the launch takes
    pointers and sizes only.  Capture succeeding is also the proof that the launch does not synchronise."""
    torch = torch_cuda
    n, B, H = 300, 3, 8
    eager, host = make(torch, n, B, H, SOA, 1)
    graphed, _ = make(torch, n, B, H, SOA, 1)
    rew, reset = scb.scripted(4, n, 1, 1, p=0.5)
    d_rew, d_reset = torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                              # warm-up on the capture stream: the code object is loaded
        graphed.step(3, d_rew, d_reset)
    torch.cuda.current_stream().wait_stream(side)
    eager.step(3, d_rew, d_reset)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step(3, d_rew, d_reset)
    fin_bin, fin_q = np.full(n, -1, np.int32), np.zeros(n, np.int64)
    host.step(np.zeros(n, np.float32), np.zeros(n, np.int64), fin_bin, fin_q)                   # the warm-up step (the capture itself runs nothing)
    for t in range(3):
        d_rew.copy_(torch.from_numpy(rew[t]))
        d_reset.copy_(torch.from_numpy(reset[t]))
        g.replay()
        eager.step(3, d_rew, d_reset)
        host.step(rew[t], reset[t], fin_bin, fin_q)
    torch.cuda.synchronize()
    assert int(eager.count.sum()) > n
    assert not scb.same_words(dev_words(torch, eager), dev_words(torch, graphed))
    assert torch.equal(eager.fin_bin, graphed.fin_bin) and torch.equal(eager.fin_q, graphed.fin_q)
    assert not scb.same_words(dev_words(torch, graphed), host.words())
