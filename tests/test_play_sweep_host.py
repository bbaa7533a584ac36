"""Sweeping physical parameters across env groups (isaacgym_amd.play: Sweep, GroupStats, Player(sweep=), include/ppenv_play_group.h) without a
GPU: the sweep's specs, grid order and tables, the per-group result arithmetic, the refusals of the three grouped entries (return code and
ppenv_last_error() text, which come from argument validation before any device call) and the CLI's parser."""
import ctypes as C
import math
import types

import numpy as np
import pytest

from isaacgym_amd import _lib

EINVAL = -1
TT_ROWS = {"dof_stiffness_scale": 7, "dof_damping_scale": 7, "link_mass_scale": 7, "restitution_scale": 0, "friction_scale": 0}
TA_ROWS = {"dof_stiffness_scale": 27, "dof_damping_scale": 27, "link_mass_scale": 28, "restitution_scale": 0, "friction_scale": 0}


# ------------------------------------------------------------------------------------------------------- Sweep
def test_parse_both_spec_forms():
    from isaacgym_amd.play import Sweep
    sw = Sweep.parse(["friction_scale=0.5:1.5:3", "restitution_scale=0.8,1.0"])
    assert len(sw) == 6
    assert sw.cells == [{"friction_scale": f, "restitution_scale": r} for f in (0.5, 1.0, 1.5) for r in (0.8, 1.0)]      # the last axis fastest
    assert Sweep.parse(["dof_stiffness_scale[5]=0.8:0.8:1"]).cells == [{"dof_stiffness_scale[5]": 0.8}]
    assert Sweep.parse(["link_mass_scale=1.3"]).cells == [{"link_mass_scale": 1.3}]
    lin = Sweep.parse(["link_mass_scale=0.7:1.3:4"]).cells
    assert [c["link_mass_scale"] for c in lin] == [float(v) for v in np.linspace(0.7, 1.3, 4)] and lin[0]["link_mass_scale"] == 0.7 and lin[-1]["link_mass_scale"] == 1.3


@pytest.mark.parametrize("spec", ["friction_scale", "friction_scale=", "=0.5", "friction_scale=a,b", "friction_scale=0.5:1.5", "friction_scale=0.5:1.5:0",
                                  "friction_scale=0.5:1.5:2.5", "friction_scale=0.5:1.5:3:4", "friction_scale=0.5,,1", "friction_scale=-1", "friction_scale=nan",
                                  "gravity=0.5,1", "friction_scale[x]=1", "friction scale=1"])
def test_parse_refuses_malformed_specs(spec):
    from isaacgym_amd.play import Sweep
    with pytest.raises(ValueError):
        Sweep.parse([spec])


def test_parse_refuses_an_axis_given_twice_and_names_the_tables():
    from isaacgym_amd.play import Sweep
    with pytest.raises(ValueError, match="twice"):
        Sweep.parse(["friction_scale=1,2", "friction_scale=3"])
    with pytest.raises(ValueError, match="dof_stiffness_scale, dof_damping_scale, link_mass_scale, restitution_scale, friction_scale"):
        Sweep.grid({"mass": [1.0]})
    with pytest.raises(ValueError):
        Sweep.grid({})
    with pytest.raises(ValueError):
        Sweep.grid({"friction_scale": []})
    with pytest.raises(ValueError, match="1..1024"):
        Sweep.grid({"friction_scale": np.linspace(0.5, 1.5, 1025)})


def test_grid_order_last_axis_fastest():
    from isaacgym_amd.play import Sweep
    sw = Sweep.grid({"link_mass_scale": [0.7, 1.3], "friction_scale": [0.5, 1.0], "restitution_scale": [0.9]})
    assert sw.cells == [{"link_mass_scale": 0.7, "friction_scale": 0.5, "restitution_scale": 0.9}, {"link_mass_scale": 0.7, "friction_scale": 1.0, "restitution_scale": 0.9},
                        {"link_mass_scale": 1.3, "friction_scale": 0.5, "restitution_scale": 0.9}, {"link_mass_scale": 1.3, "friction_scale": 1.0, "restitution_scale": 0.9}]


@pytest.mark.parametrize("rows_by_name", [TT_ROWS, TA_ROWS], ids=["7-dof", "27-dof"])
def test_tables_shapes_and_values(rows_by_name):
    """[7, N] / [27, N] / [28, N] / [N] tables; a plain axis, a row axis, a row axis over a plain one, and 1.0 where a cell names nothing."""
    from isaacgym_amd.play import Sweep
    last = rows_by_name["link_mass_scale"] - 1
    sw = Sweep([{"link_mass_scale": 1.3, "friction_scale": 0.5}, {f"link_mass_scale[{last}]": 0.7}, {"dof_stiffness_scale[5]": 0.8, "dof_stiffness_scale": 1.2}])
    N, S = 12, 4
    t = sw.tables(rows_by_name, N)
    assert sorted(t) == ["dof_stiffness_scale", "friction_scale", "link_mass_scale"]          # only the tables some cell names
    assert all(a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] for a in t.values())
    assert t["link_mass_scale"].shape == (rows_by_name["link_mass_scale"], N) and t["dof_stiffness_scale"].shape == (rows_by_name["dof_stiffness_scale"], N)
    assert t["friction_scale"].shape == (N,)
    want = np.ones((rows_by_name["link_mass_scale"], N), np.float32)
    want[:, 0:S] = 1.3
    want[last, S:2 * S] = 0.7
    assert np.array_equal(t["link_mass_scale"], want)
    assert np.array_equal(t["friction_scale"], np.array([0.5] * S + [1.0] * (2 * S), np.float32))            # unnamed cells: 1.0
    want = np.ones((rows_by_name["dof_stiffness_scale"], N), np.float32)
    want[:, 2 * S:] = 1.2
    want[5, 2 * S:] = 0.8                                                                                    # the row wins over its table's plain axis
    assert np.array_equal(t["dof_stiffness_scale"], want)


def test_tables_errors():
    from isaacgym_amd.play import Sweep
    sw = Sweep.grid({"friction_scale": [0.5, 1.0, 1.5]})
    with pytest.raises(ValueError, match=r"multiple of 3 envs, not 128.*126 and 129"):
        sw.tables(TT_ROWS, 128)
    with pytest.raises(ValueError, match=r"not 2: the nearest are 3$"):
        sw.tables(TT_ROWS, 2)
    assert sw.tables(TT_ROWS, 3)["friction_scale"].tolist() == [0.5, 1.0, 1.5]
    with pytest.raises(ValueError, match=r"link_mass_scale has 7 rows \(0\.\.6\).*'link_mass_scale': 7"):
        Sweep([{"link_mass_scale[7]": 1.1}]).tables(TT_ROWS, 4)
    assert Sweep([{"link_mass_scale[27]": 1.1}]).tables(TA_ROWS, 4)["link_mass_scale"][27].tolist() == [np.float32(1.1)] * 4
    with pytest.raises(ValueError, match=r"dof_damping_scale has 27 rows"):
        Sweep([{"dof_damping_scale[27]": 1.1}]).tables(TA_ROWS, 4)
    with pytest.raises(ValueError, match=r"friction_scale has no rows"):
        Sweep([{"friction_scale[0]": 1.1}]).tables(TT_ROWS, 4)
    with pytest.raises(ValueError, match=r"this environment's tables are dof_stiffness_scale, link_mass_scale"):
        Sweep([{"friction_scale": 1.1}]).tables({"dof_stiffness_scale": 7, "link_mass_scale": 7}, 4)
    for bad in ("mass_scale", "link_mass_scale[-1]", "link_mass_scale[1][2]", 5):
        with pytest.raises(ValueError, match="link_mass_scale, restitution_scale, friction_scale"):
            Sweep([{bad: 1.0}])
    for bad in (float("inf"), float("nan"), -0.5):
        with pytest.raises(ValueError, match="finite"):
            Sweep([{"friction_scale": bad}])


# ------------------------------------------------------------------------------------------------------- the per-group arithmetic
def _tot(x0, steps, launches):
    x0 = np.asarray(x0, np.float64)
    return dict(games=len(x0), steps=steps, launches=launches, reward=[float(x0.sum())], reward_sq=[float((x0 * x0).sum())],
                reward_min=[float(x0.min()) if len(x0) else math.inf], reward_max=[float(x0.max()) if len(x0) else -math.inf])


def test_group_summary_and_sum_on_hand_made_totals():
    from isaacgym_amd.play import group_line, group_summary, sum_totals, summarize
    xa, xb = [3.0, -1.0, 10.0, 4.0], [2.0, 6.0]
    a, b, empty = _tot(xa, 50, 20), _tot(xb, 9, 31), _tot([], 0, 31)
    ga = group_summary({"friction_scale": 0.5}, a, 1, 4)
    assert ga["cell"] == {"friction_scale": 0.5} and ga["games"] == 4 and ga["av_reward"] == 4.0 and ga["av_steps"] == 12.5 and ga["complete"] is True
    assert ga["reward_std"] == pytest.approx(np.std(xa), rel=1e-15) and ga["reward_stderr"] == ga["reward_std"] / 2.0
    assert (ga["reward_min"], ga["reward_max"]) == (-1.0, 10.0) and ga["per_agent"] == summarize(a, 1)["per_agent"]
    gb = group_summary({"friction_scale": 1.0}, b, 1, 4)
    assert gb["games"] == 2 and gb["complete"] is False and gb["reward_stderr"] == pytest.approx(2.0 / math.sqrt(2.0), rel=1e-15)
    ge = group_summary({}, empty, 1, 4)
    assert ge["games"] == 0 and ge["complete"] is False and all(math.isnan(ge[k]) for k in ("av_reward", "av_steps", "reward_std", "reward_stderr"))
    assert "games 0" in group_line(ge) and "(incomplete)" in group_line(ge) and group_line(ga).startswith("cell friction_scale=0.5: games 4 av reward 4 +- ")
    tot = sum_totals([a, b, empty])
    assert tot == dict(games=6, steps=59, launches=82, reward=[24.0], reward_sq=[166.0], reward_min=[-1.0], reward_max=[10.0])
    assert summarize(tot, 1)["av_reward"] == 4.0 and summarize(tot, 1)["av_steps"] == 59 / 6
    two = dict(games=1, steps=2, launches=2, reward=[1.0, 2.0], reward_sq=[1.0, 4.0], reward_min=[1.0, 2.0], reward_max=[1.0, 2.0])
    assert sum_totals([two, two])["reward"] == [2.0, 4.0] and len(group_summary({}, two, 2, 1)["per_agent"]) == 2


# ------------------------------------------------------------------------------------------------------- the C entries
RESET_TEXT = "pp_play_group_reset: NULL pointer, groups outside 1..1024, envs_per_group <= 0, num_agents not 1 or 2, or more than 2^31 - 1 rows"
ACC_TEXT = ("pp_play_group_accumulate: NULL pointer, groups outside 1..1024, envs_per_group <= 0, num_agents not 1 or 2, more than 2^31 - 1 rows, "
            "or games_num < 1")
P = 0x1000                      # a non-NULL pointer value: a refusal comes before anything is read or launched


def _poison(L):
    assert L.ppenv_gae(*([None] * 2 + [0, 0, None, 0, 0, 0.0, 0.0, 0.0, None, None, None])) == EINVAL      # another text in ppenv_last_error()
    return L.ppenv_last_error().decode()


def test_entries_are_bound_on_the_default_library_and_on_one_loaded_by_path(tmp_path):
    import shutil
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    for L in (_lib.lib(), _lib.load(str(shutil.copy(_lib.LIB_PATH, tmp_path / "libppenv_copy.so")))):
        assert L.pp_play_group_partial_bytes.argtypes == [i32, i32] and L.pp_play_group_partial_bytes.restype is C.c_size_t
        assert L.pp_play_group_reset.argtypes == [i32, i32, i32, vp, vp, vp, vp]
        assert L.pp_play_group_accumulate.argtypes == [vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, vp]
    assert not [n for n in vars(_lib.lib()) if n.startswith("ppenv_play_group")]          # the pinned set of ppenv_* symbols is untouched


def test_partial_bytes():
    L = _lib.lib()
    for S, G, parts in ((1, 1, 1), (256, 1, 1), (257, 1, 2), (300, 3, 6), (63, 1024, 1024), (4096, 16, 256)):
        assert L.pp_play_group_partial_bytes(S, G) == parts * 64
        assert L.pp_play_group_partial_bytes(S, 1) == L.ppenv_play_partial_bytes(S)
    for S, G in ((0, 1), (-1, 1), (1, 0), (1, 1025), (1 << 30, 2)):
        assert L.pp_play_group_partial_bytes(S, G) == 0


def test_null_is_refused_with_the_code_and_text_that_names_the_entry():
    L = _lib.lib()
    for name, text in (("pp_play_group_reset", RESET_TEXT), ("pp_play_group_accumulate", ACC_TEXT)):
        assert _poison(L) != text
        fn = getattr(L, name)
        assert fn(*[None if t is C.c_void_p else 0 for t in fn.argtypes]) == EINVAL
        assert L.ppenv_last_error().decode() == text


@pytest.mark.parametrize("S,G,A", [(0, 1, 1), (-5, 1, 1), (4, 0, 1), (4, -1, 1), (4, 1025, 1), (4, 2, 0), (4, 2, 3), (1 << 21, 1024, 1), (1 << 20, 1024, 2)])
def test_reset_refuses_sizes(S, G, A):
    L = _lib.lib()
    _poison(L)
    assert L.pp_play_group_reset(S, G, A, P, P, P, None) == EINVAL
    assert L.ppenv_last_error().decode() == RESET_TEXT


@pytest.mark.parametrize("S,G,A,games", [(0, 1, 1, 5), (4, 0, 1, 5), (4, 1025, 1, 5), (4, 2, 3, 5), (1 << 21, 1024, 1, 5), (4, 2, 1, 0), (4, 2, 2, -3)])
def test_accumulate_refuses_sizes(S, G, A, games):
    L = _lib.lib()
    _poison(L)
    assert L.pp_play_group_accumulate(P, P, S, G, A, games, P, P, P, P, None) == EINVAL
    assert L.ppenv_last_error().decode() == ACC_TEXT


@pytest.mark.parametrize("null", range(6))
def test_accumulate_refuses_each_null_pointer(null):
    L = _lib.lib()
    ptrs = [P] * 6
    ptrs[null] = None
    rew, done, cur_reward, cur_steps, totals, partial = ptrs
    _poison(L)
    assert L.pp_play_group_accumulate(rew, done, 4, 2, 1, 5, cur_reward, cur_steps, totals, partial, None) == EINVAL
    assert L.ppenv_last_error().decode() == ACC_TEXT
    if null < 3:
        _poison(L)
        assert L.pp_play_group_reset(4, 2, 1, *[None if k == null else P for k in range(3)], None) == EINVAL
        assert L.ppenv_last_error().decode() == RESET_TEXT


# ------------------------------------------------------------------------------------------------------- plumbing
def test_group_stats_and_player_argument_checks():
    import torch
    from isaacgym_amd.play import GroupStats, Player, Sweep
    for args in ((0, 2, 1, 5), (4, 0, 1, 5), (4, 1025, 1, 5), (4, 2, 3, 5), (4, 2, 1, 0), (1 << 21, 1024, 1, 5)):
        with pytest.raises(ValueError, match="GroupStats"):
            GroupStats(*args, "cuda:0")
    dev = torch.device("cuda:0")
    sw = Sweep.grid({"friction_scale": [0.5, 1.0]})
    policy = types.SimpleNamespace(device=dev, net=types.SimpleNamespace(num_obs=80, num_actions=7))
    task = types.SimpleNamespace(rl_device=dev, device=dev, num_obs=80, num_actions=7, num_envs=4, num_agents=1, randomize=True)
    with pytest.raises(ValueError, match="randomize: True"):
        Player(task, policy, sweep=sw)
    task.randomize = False
    with pytest.raises(ValueError, match="outcomes=True with a sweep"):
        Player(task, policy, sweep=sw, outcomes=True)
    task.num_envs, task.env = 5, types.SimpleNamespace(DR_TABLE_ROWS=TT_ROWS)
    with pytest.raises(ValueError, match="multiple of 2 envs, not 5"):
        Player(task, policy, sweep=sw)


def test_cli_parsing():
    from isaacgym_amd.play import Sweep, parse_args
    a = parse_args(["--checkpoint", "x.pth"])
    assert a.sweep is None and a.sweep_out is None
    a = parse_args(["--checkpoint", "x.pth", "--sweep", "friction_scale=0.5:1.5:3", "--sweep", "restitution_scale=0.8,1.0", "--sweep-out", "cells.json"])
    assert a.sweep == ["friction_scale=0.5:1.5:3", "restitution_scale=0.8,1.0"] and a.sweep_out == "cells.json"
    assert len(Sweep.parse(a.sweep)) == 6
    for bad in (["--sweep", "gravity=0.5,1"], ["--sweep", "friction_scale=1:2"], ["--sweep-out", "cells.json"],
                ["--sweep", "friction_scale=1,2", "--sweep", "friction_scale=3"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "x.pth"] + bad)
