"""RolloutCollector's observation path on CPU tensors, with stand-ins for everything that launches: which object is called in which
order, and WHICH BUFFER every tensor argument is (by identity: address and shape), for {sensing line or not} x {history or not} x
{command line or not}.  No kernel runs: the env, the network, latency.DelayLine, history.HistoryStack, critic_input.CriticInput and
collector.gae are recorders.  The sequences below are written out, not derived from the collector."""
import pytest
import torch

from isaacgym_amd import collector, critic_input
from isaacgym_amd import history as history_mod
from isaacgym_amd.latency import COMMAND

H, ROWS, NUM_OBS, NUM_ACT = 2, 4, 3, 2
HISTORY = (1, 1)                                  # rows of (1 + 1) * 3 + 1 * 2 = 8 columns


class Rig:
    """The recorders of one collector and the names of its buffers."""

    def __init__(self, monkeypatch, width):
        self.calls, self.col = [], None           # calls: (format, {argument: tensor or None}); named once the collector stands
        rig = self

        class Env:
            num_envs = num_rows = ROWS
            num_agents, device = 1, torch.device("cpu")
            obs_buf = torch.arange(1.0, ROWS * NUM_OBS + 1).reshape(ROWS, NUM_OBS)

            def step(self, act, obs=None, rew=None, reset=None):
                rig.calls.append(("env.step act={act} obs={obs} rew={rew} reset={reset}", dict(act=act, obs=obs, rew=rew, reset=reset)))

        class Net:
            num_actions, num_obs, num_priv = NUM_ACT, width, 0

            def forward(self, obs, head_out=None, sample=None, priv=None):
                rig.calls.append(("net.forward obs={obs} priv={priv}", dict(obs=obs, priv=priv)))

        class Line:
            def __init__(self, rows, width, lo, hi, device, num_agents, seed, env_id_offset, channel):
                self.name = "act_line" if channel == COMMAND else "obs_line"

            def push(self, x, done, out):
                rig.calls.append((self.name + ".push src={src} done={done} out={out}", dict(src=x, done=done, out=out)))
                return out

        class Stack:
            def __init__(self, rows, num_obs, num_actions, obs_back, actions_back, device, num_agents=1):
                assert (rows, num_obs, num_actions, obs_back, actions_back) == (ROWS, NUM_OBS, NUM_ACT) + HISTORY

            def push(self, obs, act, done, prev, out):
                rig.calls.append(("history.push seen={seen} action={action} done={done} prev={prev} out={out}",
                                  dict(seen=obs, action=act, done=done, prev=prev, out=out)))
                return out

        class Gather:
            P = 5

            def __init__(self, env, lines, names):
                pass

            def gather(self, out):
                rig.calls.append(("critic_input.gather out={out}", dict(out=out)))

        self.env, self.net = Env(), Net()
        monkeypatch.setattr(collector, "DelayLine", Line)
        monkeypatch.setattr(history_mod, "HistoryStack", Stack)
        monkeypatch.setattr(critic_input, "CriticInput", Gather)
        monkeypatch.setattr(collector, "gae", lambda *a, **k: None)

    def hook(self, name):
        rig = self

        class Hook:
            def step(self, t, rew_t, reset_t):
                rig.calls.append((name + ".step t=" + str(t) + " rew={rew} reset={reset}", dict(rew=rew_t, reset=reset_t)))
        return Hook()

    def build(self, **kw):
        self.col = collector.RolloutCollector(self.env, self.net, horizon=H, **kw)
        return self.col

    def take(self):
        """The calls recorded since the last take(), every tensor argument replaced by its buffer's name."""
        col, names = self.col, {}
        key = lambda t: (t.data_ptr(), tuple(t.shape))
        for attr in ("raw_obs", "seen_obs", "cur_obs", "applied"):
            if getattr(col, attr) is not None:
                names[key(getattr(col, attr))] = attr
        for attr in ("obs", "priv", "actions", "rewards", "dones"):
            buf = getattr(col, attr)
            for t in range(0 if buf is None else buf.shape[0]):
                names[key(buf[t])] = f"{attr}[{t}]"
        assert key(self.env.obs_buf) not in names
        out = [fmt.format(**{k: "None" if v is None else names[key(v)] for k, v in args.items()}) for fmt, args in self.calls]
        self.calls.clear()
        return out


# per configuration (sensing line, history): the calls of construction, of one collect() with a command line and without one, and the
# buffers that exist
EXPECTED = {
    (False, False): dict(
        exist=(),
        init=[],
        first="obs[0]",                           # where env.obs_buf is copied to
        lined=["net.forward obs=obs[0] priv=None",
               "act_line.push src=actions[0] done=None out=applied",
               "env.step act=applied obs=obs[1] rew=rewards[0] reset=dones[0]",
               "net.forward obs=obs[1] priv=None",
               "act_line.push src=actions[1] done=dones[0] out=applied",
               "env.step act=applied obs=obs[2] rew=rewards[1] reset=dones[1]",
               "net.forward obs=obs[2] priv=None"],
        plain=["net.forward obs=obs[0] priv=None",
               "env.step act=actions[0] obs=obs[1] rew=rewards[0] reset=dones[0]",
               "net.forward obs=obs[1] priv=None",
               "env.step act=actions[1] obs=obs[2] rew=rewards[1] reset=dones[1]",
               "net.forward obs=obs[2] priv=None"]),
    (True, False): dict(
        exist=("raw_obs",),
        init=["obs_line.push src=raw_obs done=None out=obs[0]"],
        first="raw_obs",
        lined=["net.forward obs=obs[0] priv=None",
               "act_line.push src=actions[0] done=None out=applied",
               "env.step act=applied obs=raw_obs rew=rewards[0] reset=dones[0]",
               "obs_line.push src=raw_obs done=dones[0] out=obs[1]",
               "net.forward obs=obs[1] priv=None",
               "act_line.push src=actions[1] done=dones[0] out=applied",
               "env.step act=applied obs=raw_obs rew=rewards[1] reset=dones[1]",
               "obs_line.push src=raw_obs done=dones[1] out=obs[2]",
               "net.forward obs=obs[2] priv=None"],
        plain=["net.forward obs=obs[0] priv=None",
               "env.step act=actions[0] obs=raw_obs rew=rewards[0] reset=dones[0]",
               "obs_line.push src=raw_obs done=dones[0] out=obs[1]",
               "net.forward obs=obs[1] priv=None",
               "env.step act=actions[1] obs=raw_obs rew=rewards[1] reset=dones[1]",
               "obs_line.push src=raw_obs done=dones[1] out=obs[2]",
               "net.forward obs=obs[2] priv=None"]),
    (False, True): dict(
        exist=("cur_obs",),
        init=["history.push seen=cur_obs action=None done=None prev=None out=obs[0]"],
        first="cur_obs",
        lined=["net.forward obs=obs[0] priv=None",
               "act_line.push src=actions[0] done=None out=applied",
               "env.step act=applied obs=cur_obs rew=rewards[0] reset=dones[0]",
               "history.push seen=cur_obs action=actions[0] done=dones[0] prev=obs[0] out=obs[1]",
               "net.forward obs=obs[1] priv=None",
               "act_line.push src=actions[1] done=dones[0] out=applied",
               "env.step act=applied obs=cur_obs rew=rewards[1] reset=dones[1]",
               "history.push seen=cur_obs action=actions[1] done=dones[1] prev=obs[1] out=obs[2]",
               "net.forward obs=obs[2] priv=None"],
        plain=["net.forward obs=obs[0] priv=None",
               "env.step act=actions[0] obs=cur_obs rew=rewards[0] reset=dones[0]",
               "history.push seen=cur_obs action=actions[0] done=dones[0] prev=obs[0] out=obs[1]",
               "net.forward obs=obs[1] priv=None",
               "env.step act=actions[1] obs=cur_obs rew=rewards[1] reset=dones[1]",
               "history.push seen=cur_obs action=actions[1] done=dones[1] prev=obs[1] out=obs[2]",
               "net.forward obs=obs[2] priv=None"]),
    (True, True): dict(
        exist=("raw_obs", "seen_obs"),
        init=["obs_line.push src=raw_obs done=None out=seen_obs",
              "history.push seen=seen_obs action=None done=None prev=None out=obs[0]"],
        first="raw_obs",
        lined=["net.forward obs=obs[0] priv=None",
               "act_line.push src=actions[0] done=None out=applied",
               "env.step act=applied obs=raw_obs rew=rewards[0] reset=dones[0]",
               "obs_line.push src=raw_obs done=dones[0] out=seen_obs",
               "history.push seen=seen_obs action=actions[0] done=dones[0] prev=obs[0] out=obs[1]",
               "net.forward obs=obs[1] priv=None",
               "act_line.push src=actions[1] done=dones[0] out=applied",
               "env.step act=applied obs=raw_obs rew=rewards[1] reset=dones[1]",
               "obs_line.push src=raw_obs done=dones[1] out=seen_obs",
               "history.push seen=seen_obs action=actions[1] done=dones[1] prev=obs[1] out=obs[2]",
               "net.forward obs=obs[2] priv=None"],
        plain=["net.forward obs=obs[0] priv=None",
               "env.step act=actions[0] obs=raw_obs rew=rewards[0] reset=dones[0]",
               "obs_line.push src=raw_obs done=dones[0] out=seen_obs",
               "history.push seen=seen_obs action=actions[0] done=dones[0] prev=obs[0] out=obs[1]",
               "net.forward obs=obs[1] priv=None",
               "env.step act=actions[1] obs=raw_obs rew=rewards[1] reset=dones[1]",
               "obs_line.push src=raw_obs done=dones[1] out=seen_obs",
               "history.push seen=seen_obs action=actions[1] done=dones[1] prev=obs[1] out=obs[2]",
               "net.forward obs=obs[2] priv=None"]),
}


@pytest.mark.parametrize("command", [True, False], ids=["command-line", "no-command-line"])
@pytest.mark.parametrize("sensing,stacked", list(EXPECTED), ids=["plain", "sensing-line", "history", "sensing-line-and-history"])
def test_the_observation_path_calls_and_buffers(monkeypatch, sensing, stacked, command):
    want = EXPECTED[sensing, stacked]
    rig = Rig(monkeypatch, 8 if stacked else NUM_OBS)
    col = rig.build(obs_delay=(0, 2) if sensing else 0, action_delay=1 if command else 0, history=HISTORY if stacked else None)
    for attr in ("raw_obs", "seen_obs", "cur_obs"):
        assert (getattr(col, attr) is not None) == (attr in want["exist"]), attr
    assert (col.applied is not None) == command and (col.act_line is not None) == command
    assert (col.obs_line is not None) == sensing and (col.history is not None) == stacked
    assert col.priv is None and col.critic_input is None and col._done_prev is None
    assert tuple(col.obs.shape) == (H + 1, ROWS, 8 if stacked else NUM_OBS)
    assert rig.take() == want["init"]
    first = col.obs[0] if want["first"] == "obs[0]" else getattr(col, want["first"])
    assert torch.equal(first, rig.env.obs_buf) and first.data_ptr() != rig.env.obs_buf.data_ptr()      # the initial observation: one copy
    col.collect()
    assert rig.take() == want["lined" if command else "plain"]
    assert col._done_prev.data_ptr() == col.dones[H - 1].data_ptr()
    col.collect()                                                  # the second horizon's first command push sees the first's last dones
    again = [c.replace("act_line.push src=actions[0] done=None", "act_line.push src=actions[0] done=dones[1]") for c in want["lined" if command else "plain"]]
    assert rig.take() == again


def test_the_hooks_follow_the_observation_path_in_order(monkeypatch):
    """Everything on: command line, env step, sensing push, history push, serve hook, randomizer hook, critic-input gather, on_step."""
    rig = Rig(monkeypatch, 8)
    rig.net.num_priv = 5
    col = rig.build(obs_delay=(0, 2), action_delay=1, history=HISTORY, serve=rig.hook("serve"), randomizer=rig.hook("randomizer"), critic_input=("raw_obs",))
    col.on_step = lambda: rig.calls.append(("on_step done_prev={d}", dict(d=col._done_prev)))
    assert tuple(col.priv.shape) == (H + 1, ROWS, 5)
    assert rig.take() == ["obs_line.push src=raw_obs done=None out=seen_obs",
                          "history.push seen=seen_obs action=None done=None prev=None out=obs[0]",
                          "critic_input.gather out=priv[0]"]
    col.collect()
    assert rig.take() == ["net.forward obs=obs[0] priv=priv[0]",
                          "act_line.push src=actions[0] done=None out=applied",
                          "env.step act=applied obs=raw_obs rew=rewards[0] reset=dones[0]",
                          "obs_line.push src=raw_obs done=dones[0] out=seen_obs",
                          "history.push seen=seen_obs action=actions[0] done=dones[0] prev=obs[0] out=obs[1]",
                          "serve.step t=0 rew=rewards[0] reset=dones[0]",
                          "randomizer.step t=0 rew=rewards[0] reset=dones[0]",
                          "critic_input.gather out=priv[1]",
                          "on_step done_prev=dones[0]",
                          "net.forward obs=obs[1] priv=priv[1]",
                          "act_line.push src=actions[1] done=dones[0] out=applied",
                          "env.step act=applied obs=raw_obs rew=rewards[1] reset=dones[1]",
                          "obs_line.push src=raw_obs done=dones[1] out=seen_obs",
                          "history.push seen=seen_obs action=actions[1] done=dones[1] prev=obs[1] out=obs[2]",
                          "serve.step t=1 rew=rewards[1] reset=dones[1]",
                          "randomizer.step t=1 rew=rewards[1] reset=dones[1]",
                          "critic_input.gather out=priv[2]",
                          "on_step done_prev=dones[1]",
                          "net.forward obs=obs[2] priv=priv[2]"]
