"""Paired differences (isaacgym_amd.play: PairStats, Player(paired_diff=), per-cell policies; include/ppenv_play_pair.h) without a GPU: the
host build of the kernels' per-element header against a numpy restatement of the header's rule, the algebra of swapping a cell with its
baseline, the refusals of the entries (argument validation, before any device call) and of the Python layer, the result arithmetic and
the CLI's parser.

Bounds: the table, count, len, `pairs` and the summed length difference are integers or single fp32 additions in step order: equal.
A fp64 sum of n terms: within n x 2^-52 x sum|term| of numpy's — both sides add the SAME fp64 terms (d = x - y and fl(d * d) are formed
identically), each in some order with at most (n - 1) x 2^-53 x sum|term| of rounding error."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import play_pair_shim_binding as pps
from isaacgym_amd import _lib

EINVAL = -1


def run_shim(S, G, A, M, baseline, rews, dones):
    h = pps.HostPairs(S, G, A, M, baseline)
    for t in range(rews.shape[0]):
        h.record(rews[t], dones[t])
    return h


# ------------------------------------------------------------------------------------------------------- record and reduce vs numpy
@pytest.mark.parametrize("S,G,A,M,baseline", pps.SHAPES)
def test_shim_matches_numpy(S, G, A, M, baseline):
    rews, dones = pps.streams(S, G, A)
    h = run_shim(S, G, A, M, baseline, rews, dones)
    count, ret, length = pps.numpy_record(rews, dones, S, G, A, M)
    assert h.count.tobytes() == count.tobytes() and h.len.tobytes() == length.tobytes()
    assert h.ret.tobytes() == ret.tobytes()                                                  # NaN where not played: the same bits, 0x7fc00000
    got, want = h.reduce(), pps.numpy_reduce(count, ret, length, baseline)
    for g in range(G):
        pps.check_sums(got[g], want[g], A, what=(S, G, A, M, g))
    assert sum(w["pairs"] for w in want) > 0
    if S > 3:
        assert (count[:, 3] == 0).all() and (count[:, 2] == M).all()                         # never finishes; finishes 20 times: M kept
        assert all(w["pairs"] < S * M for w in want)                                         # env 3's pairs are left out
        assert np.isnan(ret[:, 3]).all() and not np.isnan(ret[:, 2]).any()
    h.reduce()
    assert [bytes(a) for a in h.reduce()] == [bytes(a) for a in got]                         # overwritten, not accumulated


def test_table_does_not_depend_on_further_steps():
    S, G, A, M = 65, 2, 1, 1
    rews, dones = pps.streams(S, G, A, steps=80)
    full = np.ones_like(dones[0])
    h = pps.HostPairs(S, G, A, M, 0)
    h.record(rews[0], full)                                                                  # every env finishes once: the table is full
    table = h.state_bytes()[2:]
    for t in range(1, 80):
        h.record(rews[t], dones[t])
    assert h.state_bytes()[2:] == table and (h.count == M).all()


def test_integer_rewards_give_exact_sums():
    S, G, A, M = 257, 3, 2, 3
    import play_shim_binding as ps
    _, dones = pps.streams(S, G, A)
    rews = ps.rewards(pps.STEPS, S * G * A, seed=3, integer=True)
    h = run_shim(S, G, A, M, 1, rews, dones)
    want = pps.numpy_reduce(*pps.numpy_record(rews, dones, S, G, A, M), 1)
    for got, w in zip(h.reduce(), want):
        assert got.pairs == w["pairs"] and got.steps_diff == w["steps_diff"]
        for k in ("diff", "diff_sq", "cell", "base"):
            assert list(getattr(got, k)) == list(w[k]), k


# ------------------------------------------------------------------------------------------------------- algebra
@pytest.mark.parametrize("S,A,M", [(65, 2, 3), (257, 1, 1)])
def test_swapping_cell_and_baseline(S, A, M):
    rews, dones = pps.streams(S, 3, A)
    h = run_shim(S, 3, A, M, 0, rews, dones)
    fwd = h.reduce([1, 2, 0])                                                                # (copies of the structs)
    rev = h.reduce([2, 0, 1])                                                                # cell b against cell g for every (g, b) above
    for g, b in enumerate([1, 2, 0]):
        f, r = fwd[g], rev[b]
        assert f.pairs == r.pairs > 0 and f.steps_diff == -r.steps_diff
        for a in range(A):
            assert f.diff[a] == -r.diff[a] and f.diff_sq[a] == r.diff_sq[a]
            assert f.cell[a] == r.base[a] and f.base[a] == r.cell[a]
    for t in h.reduce([0, 1, 2]):                                                            # every cell against itself
        assert t.pairs > 0 and t.steps_diff == 0
        for a in range(A):
            assert t.diff[a] == 0.0 and t.diff_sq[a] == 0.0 and t.cell[a] == t.base[a]


# ------------------------------------------------------------------------------------------------------- ABI refusals
P = 0x1000                                                                                   # never dereferenced: the entries refuse first
SIZES_TEXT = "groups outside 1..1024, envs_per_group < 1, num_agents not 1 or 2, episodes < 1, or more than 2^31 - 1 table entries"
BAD_SIZES = [(4, 0, 1, 1), (4, 1025, 1, 1), (0, 2, 1, 1), (-1, 2, 1, 1), (4, 2, 0, 1), (4, 2, 3, 1), (4, 2, 1, 0), (4, 2, 1, -3),
             (1 << 20, 1024, 2, 1), (1 << 20, 1024, 1, 2), (1 << 10, 1024, 2, 1 << 10), (46341, 1, 1, 46341), (1 << 30, 1, 2, 1), (1 << 30, 4, 1, 1)]


POINTERS = {"pp_play_pair_reset": 5, "pp_play_pair_record": 7, "pp_play_pair_reduce": 5}


def _call(L, name, sizes, null=None):
    """Entry `name` with `sizes` and pointer number `null` of its pointers NULL (None: none of them) -> (rc, text).  Only ever called
    with arguments the entry must refuse: nothing is launched.  Every entry's text begins with its own name, so a text left over from
    the call before cannot pass for this call's."""
    assert null is not None or sizes in BAD_SIZES
    ptrs = [None if k == null else P for k in range(POINTERS[name])]
    if name == "pp_play_pair_record":
        rc = L.pp_play_pair_record(*ptrs[:2], *sizes, *ptrs[2:], None)
    else:
        rc = getattr(L, name)(*sizes, *ptrs, None)
    return rc, L.ppenv_last_error().decode()


@pytest.mark.parametrize("sizes", BAD_SIZES)
def test_entries_refuse_bad_sizes(sizes):
    L = _lib.lib()
    for name in POINTERS:
        assert _call(L, name, sizes) == (EINVAL, f"{name}: NULL pointer, {SIZES_TEXT}"), (name, sizes)
    assert L.pp_play_pair_ret_bytes(*sizes) == 0 and L.pp_play_pair_len_bytes(*sizes) == 0


def test_size_helpers():
    L = _lib.lib()
    assert L.pp_play_pair_ret_bytes(65, 3, 2, 3) == 65 * 3 * 2 * 3 * 4 and L.pp_play_pair_len_bytes(65, 3, 2, 3) == 65 * 3 * 3 * 4
    assert L.pp_play_pair_ret_bytes(46341, 1, 1, 46340) == 46341 * 46340 * 4                 # 2147441940 entries: under 2^31 - 1
    assert L.pp_play_pair_ret_bytes((1 << 31) - 1, 1, 1, 1) == ((1 << 31) - 1) * 4


@pytest.mark.parametrize("name,null", [(name, k) for name, n in POINTERS.items() for k in range(n)])
def test_entries_refuse_each_null_pointer(name, null):
    assert _call(_lib.lib(), name, (4, 2, 1, 3), null=null) == (EINVAL, f"{name}: NULL pointer, {SIZES_TEXT}")


# ------------------------------------------------------------------------------------------------------- Python refusals
def stand_ins(num_envs=4):
    import torch
    dev = torch.device("cuda:0")
    policy = types.SimpleNamespace(device=dev, net=types.SimpleNamespace(num_obs=80, num_actions=7))
    task = types.SimpleNamespace(rl_device=dev, device=dev, num_obs=80, num_actions=7, num_envs=num_envs, num_agents=1, randomize=False)
    return task, policy


def test_player_refusals():
    from isaacgym_amd.play import Player, Sweep
    task, policy = stand_ins()
    with pytest.raises(ValueError, match="paired_diff=True needs a sweep with paired=True"):
        Player(task, policy, paired_diff=True)
    with pytest.raises(ValueError, match="paired_diff=True needs a sweep with paired=True"):
        Player(task, policy, paired_diff=True, sweep=Sweep([{}, {}]))
    paired = Sweep([{}, {}], paired=True)
    for bad in (2, -1, [0, 2], [0], [0, 1, 0], [0.0, 1.0], "01"):
        with pytest.raises(ValueError, match="baseline"):
            Player(task, policy, paired_diff=True, sweep=paired, baseline=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="pair_episodes"):
            Player(task, policy, paired_diff=True, sweep=paired, pair_episodes=bad)
    with pytest.raises(ValueError, match="there is no sweep"):
        Player(task, [policy, policy])
    for n in (1, 3):
        with pytest.raises(ValueError, match=f"the sweep has 2 cells, the sequence {n} policies"):
            Player(task, [policy] * n, sweep=paired)
    other = types.SimpleNamespace(device=policy.device, net=types.SimpleNamespace(num_obs=80, num_actions=8))
    with pytest.raises(ValueError, match="maps 80 observations to 8 actions"):                # every policy of the sequence is checked
        Player(task, [policy, other], sweep=paired)


def test_pair_stats_refusals():
    from isaacgym_amd.play import PairStats
    for args in ((0, 2, 1, 1), (4, 0, 1, 1), (4, 1025, 1, 1), (4, 2, 3, 1), (4, 2, 1, 0), (1 << 20, 1024, 2, 1), (46341, 1, 1, 46341)):
        with pytest.raises(ValueError, match="PairStats"):
            PairStats(*args, 0, "cuda:0")
    for bad in (2, -1, [0, 2], [0, 1, 0]):
        with pytest.raises(ValueError, match="baseline"):
            PairStats(4, 2, 1, 3, bad, "cuda:0")


# ------------------------------------------------------------------------------------------------------- the result arithmetic
def hand_made(d_by_agent, x_by_agent, steps_diff):
    t = _lib.PlayPairTotals()
    t.pairs, t.steps_diff = len(d_by_agent[0]), steps_diff
    for a, (d, x) in enumerate(zip(d_by_agent, x_by_agent)):
        t.diff[a], t.diff_sq[a] = sum(d), sum(v * v for v in d)
        t.cell[a], t.base[a] = sum(x), sum(x) - sum(d)
    return t


def test_pair_summary_formula():
    from isaacgym_amd.play import pair_summary, pair_totals_dict
    d0, d1 = [1.0, 3.0, 2.0, -2.0], [0.5, 0.5, 0.5, 0.5]                                     # small integers and halves: every sum exact
    tot = pair_totals_dict(hand_made([d0, d1], [[10.0, 12.0, 8.0, 6.0], [1.0, 1.0, 1.0, 1.0]], -6), 2)
    assert tot == dict(pairs=4, steps_diff=-6, diff=[4.0, 2.0], diff_sq=[18.0, 1.0], cell_sum=[36.0, 4.0], base_sum=[32.0, 2.0])
    s = pair_summary(2, 1, tot, 2)
    assert (s["cell"], s["baseline"], s["pairs"], s["steps_diff"]) == (2, 1, 4, -1.5)
    assert s["diff"] == 1.0 and s["cell_mean"] == 9.0 and s["base_mean"] == 8.0
    assert s["diff_stderr"] == math.sqrt((18.0 - 16.0 / 4) / 3 / 4)                          # the sample variance 14 / 3 over n = 4
    assert s["diff_stderr"] == pytest.approx(np.std(d0, ddof=1) / 2.0, rel=1e-15)
    assert s["per_agent"][0] == {k: s[k] for k in ("diff", "diff_stderr", "cell_mean", "base_mean")}
    assert s["per_agent"][1] == dict(diff=0.5, diff_stderr=0.0, cell_mean=1.0, base_mean=0.5)
    assert len(pair_summary(0, 0, tot, 1)["per_agent"]) == 1
    one = pair_summary(0, 1, pair_totals_dict(hand_made([[2.5]], [[4.0]], 3), 1), 1)         # n = 1: a mean, no error bar
    assert one["diff"] == 2.5 and math.isnan(one["diff_stderr"]) and one["steps_diff"] == 3.0
    none = pair_summary(0, 1, pair_totals_dict(hand_made([[]], [[]], 0), 1), 1)
    assert none["pairs"] == 0 and all(math.isnan(none[k]) for k in ("diff", "diff_stderr", "cell_mean", "base_mean", "steps_diff"))
    same = pair_summary(1, 1, dict(pairs=130, steps_diff=0, diff=[0.0], diff_sq=[0.0], cell_sum=[7.25], base_sum=[7.25]), 1)
    assert same["diff"] == 0.0 and same["diff_stderr"] == 0.0 and same["steps_diff"] == 0.0


def test_pair_line():
    from isaacgym_amd.play import pair_line, pair_summary
    groups = [dict(cell={"friction_scale": 0.5}), dict(cell={})]
    p = pair_summary(0, 1, dict(pairs=4, steps_diff=-6, diff=[4.0], diff_sq=[18.0], cell_sum=[36.0], base_sum=[32.0]), 1)
    assert pair_line(p, groups, 4) == "cell 0 friction_scale=0.5: vs cell 1: pairs 4 diff 1 +- 1.08 (cell 9, base 8) steps diff -1.5"
    assert pair_line(p, groups, 6).endswith(" steps diff -1.5 (incomplete)")


# ------------------------------------------------------------------------------------------------------- the CLI's parser
def test_cli_parsing():
    from isaacgym_amd.play import parse_args
    base = ["--checkpoint", "x.pth"]
    a = parse_args(base)
    assert a.paired_diff is False and a.baseline is None and a.paired_out is None and a.against is None
    a = parse_args(base + ["--sweep", "friction_scale=0.5,1.0", "--paired", "--paired-diff", "--baseline", "1", "--paired-out", "d.json"])
    assert a.paired_diff and a.baseline == 1 and a.paired_out == "d.json"
    a = parse_args(base + ["--against", "y.pth", "--against", "z.pth", "--paired-out", "d.json"])
    assert a.against == ["y.pth", "z.pth"] and a.sweep is None
    a = parse_args(base + ["--against", "y.pth", "--sweep", "friction_scale=0.5,1.0", "--sweep-out", "cells.json"])
    assert a.against == ["y.pth"] and a.sweep_out == "cells.json"
    for bad in (["--paired-diff"], ["--sweep", "friction_scale=0.5,1.0", "--paired-diff"], ["--paired-out", "d.json"],
                ["--sweep", "friction_scale=0.5,1.0", "--paired", "--baseline", "1"], ["--sweep", "friction_scale=0.5,1.0", "--paired", "--paired-out", "d.json"],
                ["--against", "y.pth", "--baseline", "1"], ["--against", "y.pth", "--outcomes"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
