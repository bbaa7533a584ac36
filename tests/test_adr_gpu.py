"""ADR's launches on the MI355X (include/ppenv_dr_adr.h) against the host build of the same per-env and per-slot code
(adr_shim_binding.HostAdr), word for word, on the same streams of rewards and dones: one env, a partial last workgroup, a second workgroup of
one env, one and two rows per env, 7-dof and 27-dof row counts, one dim alone, two env-id offsets; a captured step replayed; two shards
drawing the columns and slots of the whole.  Need a real MI355X."""
import numpy as np
import pytest

import adr_shim_binding as ab
from isaacgym_amd import _lib, dr, scene
from test_play_gpu import torch_cuda        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = scene.stream_seed(9, scene.STREAM_TABLES)
U32 = np.uint32


class Handle:
    """What adr.AutoRandomizer asks of an env handle, without an env: the library, the sizes, the row counts and where the tables go."""
    dr_tables = reset_randomization = None

    def __init__(self, torch, n, dims, A, offset):
        self.L, self.device, self.num_envs, self.num_agents, self.offset = _lib.lib(), torch.device(DEV), n, A, offset
        self.DR_TABLE_ROWS = {name: (m["rows"] if m["rows"] > 1 else 0) for name, m in zip(dr.TABLE_NAMES, dims)}

    def serve_target(self):
        return dict(reset_rows=self.num_agents, env_id_offset=self.offset)

    def set_randomization(self, **tables):
        self.dr_tables = tables


def named(dims):
    return {name: dict(start=m["start"], limit=m["limit"], step=m["step"]) for name, m in zip(dr.TABLE_NAMES, dims)}


def make(torch, n, dims, H, A=1, offset=0, **kw):
    from isaacgym_amd.adr import AutoRandomizer
    env = Handle(torch, n, dims, A, offset)
    dev = AutoRandomizer(env, named(dims), seed=SEED, horizon=H, **kw)
    assert all(env.dr_tables[k] is t for k, t in dev.tables.items()) and[max(r, 1) for r in env.DR_TABLE_ROWS.values()] == dev.rows
    host = ab.HostAdr(n, dims, reset_rows=A, num_agents=A, seed=SEED, env_id_offset=offset, **kw)
    return dev, host


def dev_words(dev):
    """The device state and tables as adr_shim_binding's words() gives the host's."""
    out = {}
    for k in ab.STATE:
        t = getattr(dev, k).contiguous()
        out[k] = t.cpu().numpy().view(U32 if t.element_size() == 4 else np.uint64)
    for d, name in enumerate(dev.names):
        out[f"table{d}"] = dev.tables[name].reshape(dev.rows[d], dev.num_envs).cpu().numpy().view(U32)
    return out


@pytest.mark.parametrize("off", [0, 1000])
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("dims", list(ab.DIM_SETS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_four_launches_match_the_host_build(torch_cuda, n, dims, A, off):
    torch = torch_cuda
    H = 8
    dev, host = make(torch, n, ab.DIM_SETS[dims], H, A, off, **ab.SCRIPT_KW)
    assert not ab.same_words(dev_words(dev), host.words())                                     # fill
    assert dev.thr == host.adr.thr
    rew, reset = ab.scripted(40, n, A, A)
    d_rew, d_reset = torch.from_numpy(rew).to(DEV), torch.from_numpy(reset).to(DEV)
    fin_slot, fin_q = np.full((H, n), -1, np.int32), np.zeros((H, n), np.int64)
    games = 0
    for t in range(40):
        r = t % H
        dev.step(r, d_rew[t], d_reset[t])
        host.step(rew[t], reset[t], fin_slot[r], fin_q[r])
        diff = ab.same_words(dev_words(dev), host.words())
        assert not diff, (t, diff)
        assert np.array_equal(dev.fin_slot[r].cpu().numpy(), fin_slot[r]), t
        fired = reset[t][::A] != 0
        assert np.array_equal(dev.fin_q[r].cpu().numpy()[fired], fin_q[r][fired]), t
        if r == H - 1:
            tot = host.fold(fin_slot, fin_q)
            assert np.array_equal(dev.fold().cpu().numpy(), tot), t
            games += int(tot[0].sum())
            dev.update()
            host.update(tot)
            diff = ab.same_words(dev_words(dev), host.words())
            assert not diff, (t, "update", diff)
    assert int(host.games.sum()) == games and (games > 0 or n == 1)
    table = dev.table()
    assert np.array_equal(table["lo"].cpu().numpy(), host.range[:, 0]) and np.array_equal(table["hi"].cpu().numpy(), host.range[:, 1])
    if n in (63, 64, 65) and dims != "one":
        assert int(host.widened.sum()) >= 1 and int(host.narrowed.sum()) >= 1


def test_captured_step_replays_like_eager(torch_cuda):
    """One captured step launch replayed three times equals three eager launches: the state lives in device memory and the launch takes
    pointers and sizes only.  Capture succeeding is also the proof that the launch does not synchronise."""
    torch = torch_cuda
    n, H = 300, 8
    eager, host = make(torch, n, ab.DIMS_7, H, **ab.SCRIPT_KW)
    graphed, _ = make(torch, n, ab.DIMS_7, H, **ab.SCRIPT_KW)
    rew, reset = ab.scripted(4, n, 1, 1, p=0.5)
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
    fin_slot, fin_q = np.full(n, -1, np.int32), np.zeros(n, np.int64)
    host.step(np.zeros(n, np.float32), np.zeros(n, np.int64), fin_slot, fin_q)                  # the warm-up step (the capture itself runs nothing)
    for t in range(3):
        d_rew.copy_(torch.from_numpy(rew[t]))
        d_reset.copy_(torch.from_numpy(reset[t]))
        g.replay()
        eager.step(3, d_rew, d_reset)
        host.step(rew[t], reset[t], fin_slot, fin_q)
    torch.cuda.synchronize()
    assert int(eager.draws.sum()) > 2 * n
    assert not ab.same_words(dev_words(eager), dev_words(graphed))
    assert torch.equal(eager.fin_slot, graphed.fin_slot) and torch.equal(eager.fin_q, graphed.fin_q)
    assert not ab.same_words(dev_words(graphed), host.words())


def test_two_shards_draw_the_columns_and_slots_of_the_whole(torch_cuda):
    torch = torch_cuda
    n, cut, H = 300, 130, 8
    kw = dict(boundary_frac=0.5, min_games=1, t_low=-ab.FLT_MAX, t_high=ab.FLT_MAX)            # statistics only: the ranges stay the starts on every shard
    whole, _ = make(torch, n, ab.DIMS_7, H, offset=40, **kw)
    left, _ = make(torch, cut, ab.DIMS_7, H, offset=40, **kw)
    right, _ = make(torch, n - cut, ab.DIMS_7, H, offset=40 + cut, **kw)
    rew, reset = ab.scripted(8, n, 1, 1, p=0.4)
    d_rew, d_reset = torch.from_numpy(rew).to(DEV), torch.from_numpy(reset).to(DEV)
    for t in range(8):
        whole.step(t, d_rew[t], d_reset[t])
        left.step(t, d_rew[t, :cut].contiguous(), d_reset[t, :cut].contiguous())
        right.step(t, d_rew[t, cut:].contiguous(), d_reset[t, cut:].contiguous())
    w, a, b = dev_words(whole), dev_words(left), dev_words(right)
    for k in ("draws", "slot", "ret"):
        assert np.array_equal(w[k], np.concatenate([a[k], b[k]])), k
    for d in range(5):
        assert np.array_equal(w[f"table{d}"], np.concatenate([a[f"table{d}"], b[f"table{d}"]], axis=1)), d
    assert np.array_equal(whole.fin_slot.cpu().numpy(), np.concatenate([left.fin_slot.cpu().numpy(), right.fin_slot.cpu().numpy()], axis=1))
    tot = whole.fold().clone()
    assert torch.equal(tot, left.fold() + right.fold()) and int(tot[0].sum()) > 0              # the shards' totals sum to the whole's: what the ranks all-reduce
    assert len(set(whole.slot.tolist())) >= 6
