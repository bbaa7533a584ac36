"""The trainer's score meter (include/ppenv_ppo_meter.h) and the run loop around it, without a GPU: the kernels' arithmetic
(isaacgym_amd/csrc/ppenv_ppo_meter_device.h, compiled for the host in the kernels' summation order by tests/ppo_meter_shim_binding.py)
against rl_games' per-step loop restated in numpy below, `fit`'s decisions on a stub trainer, the train-yaml mapping of the three new
settings, and what the C entries answer to bad arguments.

Bounds.  The integers, cur_reward (one fp32 addition per env and step) and cur_len are compared for equality.  With integer-valued
rewards every return and every S_t is an integer below 2^53, so the means are compared for equality too (bitwise).  With real rewards a
fp64 sum of c_t terms, in any order, is within c_t x 2^-53 x sum|x| of the exact sum (math.fsum; the bound tests/test_play_host.py
uses); the means are then compared, for equality, after feeding the shim's own S_t through the restated update."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import play_shim_binding as ps
import ppo_meter_shim_binding as ms
from isaacgym_amd import _lib, ppo

STEPS = 64                                                             # one scripted sequence, fed in horizons of H
ENVS = [1, 63, 64, 65, 256, 257, 513]
HORIZONS = [1, 2, 32]
WINDOWS = [1, 3, 100]
WORDS = (1, 2, 1 << 32)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "task_cfgs.json")


# ---------------------------------------------------------------------------------------------------------------- the restatement
class AverageMeter:
    """rl_games' algos_torch.torch_ext.AverageMeter.update, fed one step's (sum, count) instead of the values: fp64, one rounding per
    operation (Python floats do not contract)."""

    def __init__(self, max_size):
        self.max_size, self.current_size, self.mean = int(max_size), 0, 0.0

    def update(self, total, count):
        new_mean = total / count
        size = min(count, self.max_size)
        old_size = min(self.max_size - size, self.current_size)
        size_sum = old_size + size
        self.current_size = size_sum
        self.mean = (self.mean * old_size + new_mean * size) / size_sum


class RLGamesMeters:
    """rl_games' a2c_common.play_steps bookkeeping on recorded [steps, rows] rewards and done words: float32 `current_rewards += rewards`,
    `current_lengths += 1`, `dones.nonzero()`, `all_done_indices[::num_agents]`, game_rewards.update / game_lengths.update with the
    finished envs' values, and the finished rows' running values to zero.  Restatement choices: an env finishes when AGENT 0's done word is
    non-zero, which is all_done_indices[::num_agents] whenever an env's rows carry its word together (asserted when they do); every row's
    running values restart by its own done word (rl_games multiplies by 1 - done); S_t is the exact sum (math.fsum)."""

    def __init__(self, rows, num_agents, games_to_track):
        self.A = num_agents
        self.cur, self.length = np.zeros(rows, np.float32), np.zeros(rows, np.int64)
        self.rewards, self.lengths = AverageMeter(games_to_track), AverageMeter(games_to_track)
        self.games_total = self.updates = 0
        self.steps = []                                                # per step: (exact S_t, sum|x|, L_t, c_t)

    def feed(self, rews, dones, sums=None):
        """sums: S_t per step to put through the update instead of the exact sums (the shim's own)."""
        A = self.A
        for t in range(rews.shape[0]):
            self.cur = (self.cur + rews[t]).astype(np.float32)
            self.length += 1
            all_done = np.nonzero(dones[t])[0]
            env_done = A * np.nonzero(dones[t, ::A])[0]
            if A == 1 or np.array_equal(dones[t, 0::A] != 0, dones[t, 1::A] != 0):
                assert np.array_equal(env_done, all_done[::A])
            x = [float(v) for v in self.cur[env_done]]
            c = len(x)
            exact, total_len = math.fsum(x), int(self.length[env_done].sum())
            self.steps.append((exact, math.fsum(abs(v) for v in x), total_len, c))
            if c > 0:
                self.rewards.update(exact if sums is None else float(sums[t]), c)
                self.lengths.update(float(total_len), c)
                self.games_total += c
                self.updates += 1
            self.cur[all_done] = 0.0
            self.length[all_done] = 0

    def fields(self):
        return dict(mean_reward=self.rewards.mean, mean_length=self.lengths.mean, current_size=self.rewards.current_size,
                    games_total=self.games_total, updates=self.updates)


def bits(x):
    return np.float64(x).tobytes()


def assert_fields_equal(got, want, what=""):
    for k in ("current_size", "games_total", "updates"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} vs {want[k]}"
    for k in ("mean_reward", "mean_length"):
        assert bits(got[k]) == bits(want[k]), f"{what}: {k} {got[k]!r} vs {want[k]!r}"


def sequence(num_envs, num_agents, integer, seed=0):
    rows = num_envs * num_agents
    return (ps.rewards(STEPS, rows, seed=6 + num_envs + seed, integer=integer),
            ps.scripted_dones(STEPS, num_envs, num_agents, words=WORDS, seed=5 + seed))


# ---------------------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("num_agents", [1, 2])
@pytest.mark.parametrize("num_envs", ENVS)
def test_integer_rewards_every_field_equal(num_envs, num_agents, h, w):
    rews, dones = sequence(num_envs, num_agents, integer=True)
    assert set(np.unique(dones)) <= {0, 1, 2, 1 << 32} and np.array_equal(rews, np.round(rews))
    shim, ref = ms.HostMeter(num_envs, num_agents, w), RLGamesMeters(rews.shape[1], num_agents, w)
    for t0 in range(0, STEPS, h):
        shim.update(rews[t0:t0 + h], dones[t0:t0 + h])
        ref.feed(rews[t0:t0 + h], dones[t0:t0 + h])
        what = f"after step {t0 + h}"
        assert_fields_equal(shim.read(), ref.fields(), what)
        assert shim.cur_reward.tobytes() == ref.cur[::num_agents].tobytes(), f"{what}: cur_reward"
        assert shim.cur_len.tobytes() == ref.length[::num_agents].astype(np.int32).tobytes(), f"{what}: cur_len"
    got = shim.read()
    assert got["games_total"] > 0 and 0 < got["current_size"] <= w


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("num_agents", [1, 2])
@pytest.mark.parametrize("num_envs", ENVS)
def test_real_rewards(num_envs, num_agents, h, w):
    rews, dones = sequence(num_envs, num_agents, integer=False)
    shim, ref = ms.HostMeter(num_envs, num_agents, w), RLGamesMeters(rews.shape[1], num_agents, w)
    for t0 in range(0, STEPS, h):
        shim.update(rews[t0:t0 + h], dones[t0:t0 + h])
        s, l, c = shim.steps
        ref.feed(rews[t0:t0 + h], dones[t0:t0 + h], sums=s)            # the shim's own S_t through the restated update
        for j in range(h):
            exact, mag, want_len, want_c = ref.steps[t0 + j]
            assert (int(l[j]), int(c[j])) == (want_len, want_c), f"step {t0 + j}: L_t, c_t"
            bound = want_c * 2.0 ** -53 * mag
            assert abs(s[j] - exact) <= bound, f"step {t0 + j}: S_t {s[j]!r} vs {exact!r}, bound {bound:.3g}"
        assert_fields_equal(shim.read(), ref.fields(), f"after step {t0 + h}")
        assert shim.cur_reward.tobytes() == ref.cur[::num_agents].tobytes()
        assert shim.cur_len.tobytes() == ref.length[::num_agents].astype(np.int32).tobytes()


def test_more_finishes_in_one_step_than_the_window():
    num_envs, w = 257, 3
    rews, dones = sequence(num_envs, 1, integer=True)
    counts = (dones != 0).sum(1)
    t = int(np.argmax(counts))
    assert counts[t] >= num_envs // 4 > w                              # the burst
    shim, ref = ms.HostMeter(num_envs, 1, w), RLGamesMeters(num_envs, 1, w)
    shim.update(rews[:t + 1], dones[:t + 1])
    ref.feed(rews[:t + 1], dones[:t + 1])
    got = shim.read()
    assert_fields_equal(got, ref.fields())
    exact, _, total_len, c = ref.steps[t]
    assert got["current_size"] == w and c > w                         # old = 0: the means are that step's alone
    assert bits(got["mean_reward"]) == bits((0.0 + exact / c * w) / w) and bits(got["mean_length"]) == bits((0.0 + total_len / c * w) / w)


def test_a_horizon_without_a_finish_changes_nothing():
    num_envs, h = 65, 32
    rews = ps.rewards(h, num_envs)
    none = np.zeros((h, num_envs), np.int64)
    shim = ms.HostMeter(num_envs, 1, 100)
    shim.update(rews, none)
    assert shim.meter.tobytes() == bytes(40) and shim.read()["current_size"] == 0
    assert np.array_equal(shim.cur_len, np.full(num_envs, h, np.int32))
    rews2, dones2 = sequence(num_envs, 1, integer=False)
    shim.update(rews2[:h], dones2[:h])
    before = shim.meter.tobytes()
    assert shim.read()["current_size"] > 0
    shim.update(rews, none)
    assert shim.meter.tobytes() == before                              # bit for bit, `updates` included


def test_a_done_on_agent_1_alone_does_not_count():
    num_envs, h = 33, 8
    rews = ps.rewards(h, 2 * num_envs, integer=True)
    dones = np.zeros((h, 2 * num_envs), np.int64)
    dones[:, 1::2] = 1
    shim, ref = ms.HostMeter(num_envs, 2, 3), RLGamesMeters(2 * num_envs, 2, 3)
    shim.update(rews, dones)
    ref.feed(rews, dones)
    assert shim.meter.tobytes() == bytes(40) and ref.fields()["games_total"] == 0
    assert np.array_equal(shim.cur_len, np.full(num_envs, h, np.int32))
    assert shim.cur_reward.tobytes() == rews[:, 0::2].sum(0, dtype=np.float32).tobytes()      # integers: exact in any order
    dones[3, 0] = 1 << 32                                              # ... and agent 0's row does
    shim = ms.HostMeter(num_envs, 2, 3)
    shim.update(rews, dones)
    got = shim.read()
    assert (got["games_total"], got["current_size"], got["mean_length"]) == (1, 1, 4.0)
    assert got["mean_reward"] == float(rews[:4, 0].sum(dtype=np.float64))


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("num_envs,num_agents,h", [(257, 1, 32), (65, 2, 32), (513, 1, 2), (1, 1, 1)])
def test_two_horizons_in_one_call_are_two_calls(num_envs, num_agents, h, integer):
    rews, dones = sequence(num_envs, num_agents, integer)
    a, b = ms.HostMeter(num_envs, num_agents, 3), ms.HostMeter(num_envs, num_agents, 3)
    a.update(rews[:h], dones[:h])
    a.update(rews[h:2 * h], dones[h:2 * h])
    b.update(rews[:2 * h], dones[:2 * h])
    assert a.state_bytes() == b.state_bytes()
    if h > 1:
        assert a.read()["games_total"] > 0 and a.cur_len.max() > h    # a game that runs across the boundary: the carry of cur_*


def test_row_strided_views_read_the_same_words():
    num_envs, num_agents, h = 65, 2, 32
    rews, dones = sequence(num_envs, num_agents, integer=False)
    wide_r = np.full((h, rews.shape[1] + 7), 1e9, np.float32)
    wide_d = np.full((h, rews.shape[1] + 7), 1, np.int64)
    wide_r[:, :rews.shape[1]], wide_d[:, :rews.shape[1]] = rews[:h], dones[:h]
    a, b = ms.HostMeter(num_envs, num_agents, 100), ms.HostMeter(num_envs, num_agents, 100)
    a.update(rews[:h], dones[:h])
    b.update(wide_r[:, :rews.shape[1]], wide_d[:, :rews.shape[1]])
    assert a.state_bytes() == b.state_bytes()


# ---------------------------------------------------------------------------------------------------------------- fit
class StubTrainer:
    """What fit() uses of a PPOTrainer, with scripted scores: script[epoch - 1] = (meter_return, meter_games)."""
    rank = 0

    def __init__(self, script, cfg):
        self.script, self.cfg = script, cfg
        self.epoch = self.frame = 0
        self.last_mean_rewards = ppo.NO_SCORE
        self.saved = []                                                # (epoch, file name, last_mean_rewards at the save)

    def train_epoch(self):
        score, games = self.script[self.epoch]
        self.epoch += 1
        self.frame += 64
        out = {k: torch.tensor(0.5) for k in ppo.STATS + ("scale", "grad_norm", "mean_return", "mean_length")}
        out.update(skipped=torch.tensor(0), episodes=torch.tensor(3.0), meter_return=torch.tensor(score, dtype=torch.float64),
                   meter_length=torch.tensor(17.0, dtype=torch.float64), meter_games=torch.tensor(games))
        return out

    def state_dict(self):
        return {"epoch": self.epoch, "frame": self.frame, "last_mean_rewards": float(self.last_mean_rewards)}

    def save(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(self.state_dict(), path)
        self.saved.append((self.epoch, os.path.basename(path), self.last_mean_rewards))

    def load(self, path):
        ck = torch.load(path, weights_only=True)
        self.epoch, self.frame, self.last_mean_rewards = ck["epoch"], ck["frame"], ck["last_mean_rewards"]


SCRIPT = [(10.0, 5), (8.0, 5), (8.0, 5), (9.0, 0), (7.0, 5), (12.5, 5), (60.25, 5), (99.0, 5)]


def test_fit_decisions(tmp_path, capsys):
    cfg = ppo.PPOConfig(save_best_after=2, score_to_win=50.0, save_frequency=3, max_epochs=8)
    tr = StubTrainer(SCRIPT, cfg)
    res = ppo.fit(tr, str(tmp_path), "T", print_every=2)
    assert tr.saved == [
        # epoch 1: 10 is a best, but before save_best_after
        (2, "T_best.pth", 8.0),                                       # the first best from save_best_after on
        # epoch 3: 8 again: only a strict improvement is a best
        (3, "T.pth", 8.0),                                            # save_frequency
        # epoch 4: 9 with meter_games == 0: nothing;  epoch 5: worse
        (6, "T_best.pth", 12.5), (6, "T.pth", 12.5),
        (7, "T_best.pth", 60.25), (7, "T_ep_7_rew_60.25.pth", 60.25), (7, "T.pth", 60.25)]     # above score_to_win: the third file, the end
    nn = tmp_path / "nn"
    assert res["epochs"] == 7 and res["epoch"] == 7 and res["stopped"] and res["reason"] == "score_to_win" and res["best_score"] == 60.25
    assert res["paths"] == dict(latest=str(nn / "T.pth"), best=str(nn / "T_best.pth"), won=str(nn / "T_ep_7_rew_60.25.pth"))
    assert res["written"] == [str(nn / name) for _, name, _ in tr.saved]
    assert sorted(os.listdir(nn)) == ["T.pth", "T_best.pth", "T_ep_7_rew_60.25.pth"]
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch ")]
    assert [l.split()[1] for l in lines] == ["2", "4", "6", "7"] and lines[-1].endswith("score 60.25 (5 games)")


def test_fit_runs_to_max_epochs_and_saves_the_latest_at_the_end(tmp_path):
    cfg = ppo.PPOConfig(save_best_after=100, score_to_win=50.0, save_frequency=1500, max_epochs=200000)
    tr = StubTrainer(SCRIPT, cfg)
    res = ppo.fit(tr, str(tmp_path), "T", print_every=0, max_epochs=4)
    assert tr.saved == [(4, "T.pth", ppo.NO_SCORE)]
    assert (res["epochs"], res["stopped"], res["reason"], res["best_score"]) == (4, False, "max_epochs", ppo.NO_SCORE) and ppo.NO_SCORE == -100500.0
    assert res["paths"]["best"] is None and res["paths"]["won"] is None
    assert ppo.fit(tr, str(tmp_path), "T", print_every=0, max_epochs=4)["epochs"] == 0       # max_epochs is the total


def test_fit_resumed_keeps_the_best_score(tmp_path):
    """last_mean_rewards travels through the checkpoint: the resumed run does not overwrite _best.pth with a worse score."""
    script = [(3.0, 5), (8.0, 5), (6.0, 5), (5.0, 5), (9.0, 5)]
    cfg = ppo.PPOConfig(save_best_after=1, save_frequency=1500)
    a = StubTrainer(script, cfg)
    ppo.fit(a, str(tmp_path), "T", print_every=0, max_epochs=3)
    latest, best = tmp_path / "nn" / "T.pth", tmp_path / "nn" / "T_best.pth"
    assert torch.load(best)["epoch"] == 2 and torch.load(latest) == dict(epoch=3, frame=192, last_mean_rewards=8.0)
    b = StubTrainer(script, cfg)
    b.load(str(latest))
    assert b.last_mean_rewards == 8.0
    res = ppo.fit(b, str(tmp_path), "T", print_every=0, max_epochs=4)
    assert (res["epochs"], res["epoch"], res["paths"]["best"]) == (1, 4, None) and torch.load(best)["epoch"] == 2     # 5 < 8: kept
    res = ppo.fit(b, str(tmp_path), "T", print_every=0, max_epochs=5)
    assert res["best_score"] == 9.0 and torch.load(best) == dict(epoch=5, frame=320, last_mean_rewards=9.0)
    fresh = StubTrainer(script, cfg)                                   # without the checkpoint the worse score would have been a best
    fresh.epoch = 3
    assert ppo.fit(fresh, str(tmp_path / "fresh"), "T", print_every=0, max_epochs=4)["paths"]["best"] is not None


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_from_train_cfg_maps_the_score_settings():
    with open(GOLDEN) as fh:
        d = json.load(fh)["HumanoidPingpongTiltG1"]
    c = ppo.PPOConfig.from_train_cfg(d["train"], task_cfg=d["task"], minibatch_size=8192)
    assert (c.score_to_win, c.save_best_after, c.games_to_track) == (20000.0, 3000, 100)
    assert isinstance(c.score_to_win, float) and isinstance(c.save_best_after, int)
    c = ppo.PPOConfig.from_train_cfg(d["train"], minibatch_size=8192, score_to_win="150", save_best_after=7, games_to_track=20)
    assert (c.score_to_win, c.save_best_after, c.games_to_track) == (150.0, 7, 20)
    t = json.loads(json.dumps(d["train"]))
    t["params"]["config"]["games_to_track"] = 50
    assert ppo.PPOConfig.from_train_cfg(t, minibatch_size=8192).games_to_track == 50
    for bad in (0, -3):
        with pytest.raises(ValueError, match=r"games_to_track"):
            ppo.PPOConfig.from_train_cfg(d["train"], minibatch_size=8192, games_to_track=bad)
        with pytest.raises(ValueError, match=r"games_to_track"):
            ppo.PPOConfig(games_to_track=bad).check()
    assert (ppo.PPOConfig().games_to_track, ppo.PPOConfig().save_best_after, ppo.PPOConfig().score_to_win) == (100, 3000, 20000.0)


def test_cli_flags():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "isaacgym_amd.ppo", "--help"], capture_output=True, text=True, timeout=120,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0
    for flag in ("--checkpoint", "--save-best-after", "--score-to-win", "--games-to-track"):
        assert flag in r.stdout, flag


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layout_and_binding():
    m = _lib.PPOMeter
    assert C.sizeof(m) == 40
    assert (m.mean_reward.offset, m.mean_length.offset, m.current_size.offset, m.games_total.offset, m.updates.offset) == (0, 8, 16, 24, 32)
    assert ppo.PPOMeter is m
    ms.lib()                                                           # asserts the compiled sizes
    L = _lib.lib()
    assert L.ppo_meter_update.argtypes is not None and len(L.ppo_meter_update.argtypes) == 13
    assert L.ppo_meter_partial_bytes.restype is C.c_size_t
    assert L.ppo_meter_partial_bytes(32, 4096) == 32 * 16 * 24 and L.ppo_meter_partial_bytes(1, 257) == 2 * 24
    assert L.ppo_meter_partial_bytes(0, 64) == 0 and L.ppo_meter_partial_bytes(4, 0) == 0 and L.ppo_meter_partial_bytes(-1, -1) == 0


GOOD = dict(rew=0x1000, ld_rew=128, done=0x2000, ld_done=128, h=32, num_envs=64, num_agents=2, games_to_track=100, cur_reward=0x3000,
            cur_len=0x4000, meter=0x5000, partial=0x6000, stream=None)


@pytest.mark.parametrize("bad", [dict(rew=None), dict(done=None), dict(cur_reward=None), dict(cur_len=None), dict(meter=None), dict(partial=None),
                                 dict(h=0), dict(num_envs=0), dict(num_envs=-5), dict(num_agents=0), dict(num_agents=3), dict(games_to_track=0),
                                 dict(ld_rew=127), dict(ld_done=127), dict(num_envs=(1 << 31) - 1, ld_rew=1 << 40, ld_done=1 << 40)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_arguments_are_refused_before_any_launch(bad):
    """Validation alone answers, before the entry touches the HIP runtime: the (never dereferenced) pointers are made up."""
    L = _lib.lib()
    assert L.ppenv_gae(*([None] * 2 + [0, 0] + [None] + [0, 0] + [0.0] * 3 + [None] * 3)) == -1      # another text in ppenv_last_error()
    assert not L.ppenv_last_error().decode().startswith("ppo_meter_update")
    assert L.ppo_meter_update(*dict(GOOD, **bad).values()) == -1                                     # PPENV_EINVAL
    assert L.ppenv_last_error().decode() == ("ppo_meter_update: NULL pointer, h < 1, num_envs < 1, num_agents not 1 or 2, more than 2^31 - 1 rows, "
                                             "a row stride below num_agents x num_envs, or games_to_track < 1")


def test_game_meter_refuses_bad_sizes():
    for args in ((0, 1, 100), (64, 3, 100), (64, 1, 0)):
        with pytest.raises(ValueError, match="GameMeter"):
            ppo.GameMeter(*args, "cpu")
