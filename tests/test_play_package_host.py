"""isaacgym_amd.play as a package (accounting, report, sweep, player, cli) without a GPU: its import surface, the
split of a Sweep's cells by kind of axis and the questions the Player asks of it, and the two helpers the accounting classes and the
summaries share."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from isaacgym_amd import _lib, play

# every public name of isaacgym_amd.play, typed in: tests, tools, ppo.py and the README import from the package, not from its files
SURFACE = ("ACT_INT_FIELDS", "ACT_MAX_FIELDS", "ACT_SUM_FIELDS", "ACT_THRESHOLDS", "ActuatorStats", "DELAY_AXES", "DELAY_MAX", "DELAY_MAX_WIDTH", "Delay",
           "EpisodeStats", "GroupStats", "MAX_AGENTS", "MAX_GROUPS", "OUTCOME_PRINTS", "PairStats", "PlayPairTotals", "PlayTotals", "Player", "SERVE_AXES",
           "Sweep", "TABLE_NAMES", "TAOutcome", "TA_OUTCOME_NAMES", "act_totals_dict", "actuator_limits", "actuator_option", "actuator_summary",
           "actuator_table", "baseline_cells", "cell_text", "control_dt_of", "delay_steps", "group_line", "group_summary", "latency_line", "main",
           "make_recorder", "make_renderer", "outcome_lines", "outcomes_dict", "pair_line", "pair_summary", "pair_totals_dict", "parse_args", "serve",
           "sum_act_totals", "sum_totals", "summarize", "totals_dict")


def test_the_package_exports_its_whole_surface():
    assert len(set(SURFACE)) == 49
    for name in SURFACE:
        exec(f"from isaacgym_amd.play import {name}", {})
    assert play.PlayTotals is _lib.PlayTotals and play.PlayPairTotals is _lib.PlayPairTotals and play.TAOutcome is _lib.TAOutcome
    assert play.MAX_GROUPS == 1024 and (play.DELAY_MAX, play.DELAY_MAX_WIDTH) == (15, 512) and play.DELAY_AXES == ("action_delay", "obs_delay")
    from isaacgym_amd.play import accounting, cli, player, report, sweep
    assert play.Player is player.Player and play.Sweep is sweep.Sweep and play.main is cli.main and play.Delay is accounting.Delay
    assert play.summarize is report.summarize and play.__doc__.startswith("Play a checkpoint")


def test_python_dash_m_runs_the_cli():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, "-m", "isaacgym_amd.play", "--help"], cwd=root, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert done.stdout.startswith("usage: python -m isaacgym_amd.play") and "--against" in done.stdout


# ------------------------------------------------------------------------------------------------------- Sweep: the cells by kind
MIXED = [{"link_mass_scale": 0.5, "link_mass_scale[2]": 2, "serve_speed": 8, "action_delay": 2.0},
         {"link_mass_scale[2]": 0.25, "link_mass_scale": 1.5, "serve_tilt": (-2, 3), "obs_delay": np.int64(1), "action_delay": 0},
         {}]
ROWS = {"link_mass_scale": 4, "friction_scale": 0}
DEFAULTS = {"serve_speed": (7.0, 9.0), "serve_tilt": (-3.0, 3.0), "serve_tilt_z": (-1.0, 1.0)}


def test_sweep_splits_its_cells_by_kind_of_axis():
    sw = play.Sweep(MIXED, paired=True)
    assert sw.cells == [{"link_mass_scale": 0.5, "link_mass_scale[2]": 2.0, "serve_speed": 8.0, "action_delay": 2},
                        {"link_mass_scale[2]": 0.25, "link_mass_scale": 1.5, "serve_tilt": (-2.0, 3.0), "obs_delay": 1, "action_delay": 0}, {}]
    assert [list(c) for c in sw.cells] == [list(c) for c in MIXED]                                      # the axes in the order they were given
    assert [type(v) for v in sw.cells[0].values()] == [float, float, float, int] and type(sw.cells[1]["obs_delay"]) is int
    assert sw.cell_tables == [[("link_mass_scale", "link_mass_scale", None, 0.5), ("link_mass_scale[2]", "link_mass_scale", 2, 2.0)],
                              [("link_mass_scale[2]", "link_mass_scale", 2, 0.25), ("link_mass_scale", "link_mass_scale", None, 1.5)], []]
    assert sw.cell_serves == [{"serve_speed": 8.0}, {"serve_tilt": (-2.0, 3.0)}, {}]
    assert sw.cell_latency == [{"action_delay": 2}, {"obs_delay": 1, "action_delay": 0}, {}]
    tables = sw.tables(ROWS, 6)                                                                         # S = 2 envs per cell
    assert list(tables) == ["link_mass_scale"] and tables["link_mass_scale"].dtype == np.float32
    want = np.ones((4, 6), np.float32)
    want[:, 0:2], want[:, 2:4] = 0.5, 1.5
    want[2, 0:2], want[2, 2:4] = 2.0, 0.25                             # the row axis wins in its row, also where the cell names it first
    assert np.array_equal(tables["link_mass_scale"], want)
    full = dict(DEFAULTS)
    assert sw.serve_cells(DEFAULTS) == [dict(full, serve_speed=(8.0, 8.0)), dict(full, serve_tilt=(-2.0, 3.0)), full]
    assert all(set(c) == set(DEFAULTS) for c in sw.serve_cells(DEFAULTS))
    assert sw.cell_delays() == dict(action_delay=[2, 0, 0], obs_delay=[0, 1, 0])
    assert sw.cell_delays(action_delay=3, obs_delay=4) == dict(action_delay=[2, 0, 3], obs_delay=[4, 1, 4])
    one, two = sw.delays(6, 1), sw.delays(6, 2, action_delay=3, obs_delay=4)
    assert all(v.dtype == np.int32 for v in list(one.values()) + list(two.values())) and list(one) == list(two) == ["action_delay", "obs_delay"]
    assert one["action_delay"].tolist() == [2, 2, 0, 0, 0, 0] and one["obs_delay"].tolist() == [0, 0, 1, 1, 0, 0]
    assert two["action_delay"].tolist() == [2] * 4 + [0] * 4 + [3] * 4 and two["obs_delay"].tolist() == [4] * 4 + [1] * 4 + [4] * 4
    assert (sw.sets_randomization, sw.needs_serve_plan, sw.has_latency) == (True, True, True)


@pytest.mark.parametrize("cells, paired, want", [
    ([{}, {}], False, (True, False, False)),                           # about nothing: still set_randomization() with no tables, the table-reading kernel
    ([{}, {}], True, (False, True, False)),                            # paired alone: a serve plan, the plain kernel
    ([{"serve_speed": 8.0}, {}], False, (False, True, False)),         # serves alone
    ([{"action_delay": 1}, {}], False, (False, False, True)),          # latency alone
    ([{"action_delay": 1}, {"friction_scale": 1.0}], True, (True, True, True))],
    ids=["empty", "empty-paired", "serve-only", "latency-only", "all-three"])
def test_what_the_player_asks_of_a_sweep(cells, paired, want):
    sw = play.Sweep(cells, paired=paired)
    assert (sw.sets_randomization, sw.needs_serve_plan, sw.has_latency) == want
    assert bool(sw.tables(ROWS, 4)) == any(sw.cell_tables) and (sw.serve_cells(DEFAULTS) is not None) == sw.needs_serve_plan
    assert sw.sets_randomization == (bool(sw.tables(ROWS, 4)) or (sw.serve_cells(DEFAULTS) is None and not sw.has_latency))    # the rule, spelled out on what the methods return


def test_cell_delays_is_one_function_with_and_without_a_sweep():
    from isaacgym_amd.play.sweep import cell_delays
    assert cell_delays([{}]) == dict(action_delay=[0], obs_delay=[0]) and cell_delays([{}], 2.0, 15) == dict(action_delay=[2], obs_delay=[15])
    sw = play.Sweep(MIXED)
    assert cell_delays(sw.cells, 3, 4) == sw.cell_delays(3, 4)
    with pytest.raises(ValueError, match="'obs_delay'.*whole control steps"):
        cell_delays([{}], obs_delay=16)


# ------------------------------------------------------------------------------------------------------- the shared helpers
def test_stderr_of_mean_is_both_summaries_expression():
    from isaacgym_amd.play.report import _stderr_of_mean
    cases = [(0.0, 0.0, 0), (3.0, 9.0, 1), (3.0, 5.0, 2), (40.0, 440.0, 4), (-7.5, 30.25, 3), (1e8 + 1.0, (1e8 + 1.0) ** 2 / 3 * (1 - 1e-15), 3),
             (0.3, 0.1 * 0.1 * 3, 3), (12.0, 36.0, 4)]
    assert any(n >= 2 and sq - s * s / n < 0.0 for s, sq, n in cases)                                     # a negative variance estimate is among them
    for s, sq, n in cases:
        pair = math.sqrt(max(sq - s * s / n, 0.0) / (n - 1) / n) if n >= 2 else float("nan")            # pair_summary's diff_stderr, written out
        got = _stderr_of_mean(s, sq, n)
        assert (math.isnan(got) and math.isnan(pair) and n < 2) or got == pair, (s, sq, n)
        dt = 0.0125
        act = dt * math.sqrt(max(sq - s * s / n, 0.0) / (n - 1) / n) if n >= 2 else float("nan")        # actuator_summary's energy_stderr, written out
        tot = dict(games=n, samples=0, energy=s, energy_sq=sq, **{k: [] for k in play.ACT_INT_FIELDS + play.ACT_SUM_FIELDS + play.ACT_MAX_FIELDS})
        got = play.actuator_summary(tot, [], [], dt)["energy_stderr"]
        assert (math.isnan(got) and math.isnan(act) and n < 2) or got == act, (s, sq, n)
        got = play.pair_summary(0, 0, dict(pairs=n, steps_diff=0, diff=[s], diff_sq=[sq], cell_sum=[0.0], base_sum=[0.0]))["diff_stderr"]
        assert (math.isnan(got) and n < 2) or got == pair, (s, sq, n)
    assert _stderr_of_mean(12.0, 36.0, 4) == 0.0


def test_read_structs_reads_a_byte_tensor_of_play_totals():
    import torch
    from isaacgym_amd.play.accounting import _read_structs
    T = play.PlayTotals
    src = (T * 3)()
    for i, t in enumerate(src):
        t.games, t.steps, t.launches = i + 1, 10 * i, 100 + i
        t.reward[0], t.reward[1], t.reward_sq[0], t.reward_min[0], t.reward_max[1] = 1.5 * i, -0.0, 2.25 * i, -math.inf, math.inf
    buf = torch.frombuffer(bytearray(bytes(src)), dtype=torch.uint8)
    assert buf.numel() == 3 * C.sizeof(T) == 3 * 72
    got = _read_structs(T, buf, 3)
    assert len(got) == 3 and all(type(t) is T for t in got) and [bytes(t) for t in got] == [bytes(t) for t in src]
    assert [play.totals_dict(t, 2) for t in got] == [play.totals_dict(t, 2) for t in src] and got[2].games == 3 and got[1].reward_sq[0] == 2.25
    assert math.copysign(1.0, got[0].reward[1]) == -1.0                                                   # bytes, not values: -0.0 stays -0.0
    assert _read_structs(T, buf[:72], 1)[0].launches == 100 and _read_structs(T, buf, 0) == []
