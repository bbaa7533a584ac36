"""The Player's options together on the MI355X: a paired sweep of physics x command latency with paired_diff, actuators and obs_delay at
once against the same sweep without paired_diff and actuators.  Player's docstring promises, option by option, that `groups`, the summed
figures and the accounting's bytes are those of the run without the option; the other GPU tests check the options one at a time."""
import pytest

from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (two fixtures, two helpers)

pytestmark = pytest.mark.gpu

TT = "HumanoidPingpongTiltG1"
CLOCK = ("steps_played", "seconds", "paired_diff", "actuators")     # what paired_diff may lengthen, and what the two options add


def test_paired_diff_and_actuators_leave_the_swept_result_alone(torch_cuda, checkpoint):
    from isaacgym_amd.play import GroupStats, Player, Sweep
    path = checkpoint(TT)

    def player(**kw):
        sweep = Sweep.grid({"friction_scale": [0.5, 1.0], "action_delay": [0, 2]}, paired=True)              # 4 cells of 16 envs
        return Player(make_plain(TT, 64, 21), load_policy(path), games_num=4, poll_every=8, max_steps=400, sweep=sweep, obs_delay=1, **kw)

    both, bare = player(paired_diff=True, actuators=True), player()
    assert type(both.stats) is GroupStats and bare.pairs is None and bare.act is None
    res, res0 = both.run(), bare.run()
    assert [g["cell"] for g in res["groups"]] == [{"friction_scale": f, "action_delay": k} for f in (0.5, 1.0) for k in (0, 2)]
    assert all(g["complete"] and g["paired"] and g["games"] >= 4 for g in res["groups"])
    assert res["groups"] == res0["groups"]
    assert {k: v for k, v in res.items() if k not in CLOCK} == {k: v for k, v in res0.items() if k not in CLOCK}
    assert set(res) - set(res0) == {"paired_diff", "actuators"} and res["steps_played"] >= res0["steps_played"]
    assert both.stats.state_bytes() == bare.stats.state_bytes()
    assert res["latency"] == dict(control_dt=both.task.env.control_dt, action_delay=[0, 2, 0, 2], obs_delay=[1, 1, 1, 1]) == res0["latency"]
    pd = res["paired_diff"]
    assert pd["episodes"] == both.pair_episodes == 1 and pd["complete"] and [(p["cell"], p["baseline"], p["pairs"]) for p in pd["cells"]] == [(g, 0, 16) for g in range(4)]
    assert pd["cells"][0]["diff"] == 0.0 and pd["cells"][0]["diff_stderr"] == 0.0
    assert all(p["diff_stderr"] >= 0.0 and p["diff"] == p["per_agent"][0]["diff"] and len(p["per_agent"]) == 1 for p in pd["cells"])
    act = res["actuators"]
    assert len(act["groups"]) == 4 and [g["cell"] for g in act["groups"]] == [g["cell"] for g in res["groups"]]
    assert [g["games"] for g in act["groups"]] == [g["games"] for g in res["groups"]] and act["total"]["games"] == res["games"]
    assert all(len(g["per_joint"]) == 7 and g["samples"] > 0 for g in act["groups"]) and len(act["joints"]) == 7
