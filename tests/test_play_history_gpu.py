"""Playing a checkpoint that carries an observation and action history on the MI355X (play.Player; history.HistoryStack;
include/ppenv_history.h): the wide rows the policy reads follow the rule step by step across resets; a plain checkpoint plays byte for
byte as the loop without any history object; a history checkpoint plays A/B against a plain one in one paired pass; a policy whose base
width is not the task's is refused.  64 envs, 12-step games, 40 control steps.  Need a real MI355X."""
import numpy as np
import pytest

from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (helpers, fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TT = "HumanoidPingpongTiltG1"
SEED, STEPS = 9, 40


@pytest.fixture(scope="module")
def history_checkpoint(torch_cuda, tmp_path_factory):
    """A checkpoint of a PPOTrainer-initialised network with history (2, 2) on the 7-dof task -> (path, record)."""
    from isaacgym_amd import ppo
    tr = ppo.PPOTrainer(make_plain(TT, 64, SEED), ppo.PPOConfig(horizon_length=4, minibatch_size=64), seed=SEED, history=(2, 2))
    path = str(tmp_path_factory.mktemp("play_history") / "history.pth")
    tr.save(path)
    return path, tr.history()


def test_wide_rows_follow_the_rule_across_resets(torch_cuda, history_checkpoint):
    torch = torch_cuda
    from isaacgym_amd import history, play
    path, rec = history_checkpoint
    pol = load_policy(path)
    assert pol.history == rec and pol.base_num_obs == rec["num_obs"] and pol.net.num_obs == rec["width"]
    task = make_plain(TT, 64, SEED)
    n, a, W = task.num_obs, task.num_actions, rec["width"]
    player = play.Player(task, pol, games_num=10 ** 6, max_steps=STEPS)
    assert list(player._stacks) == [(2, 2)] and player.history() == [rec]
    for again in range(2):                                     # start() resets the stack: the first push starts every row again
        player.start()
        prev_wide = prev_act = None
        resets = carried = 0
        for t in range(STEPS):
            seen = player._obs.clone()
            done_prev = None if player._done_prev is None else player._done_prev.clone()
            player.step()
            wide, act = player.policy_obs.clone(), player.actions.clone()
            assert wide.shape == (64, W) and torch.equal(wide[:, :n].view(torch.int32), seen.view(torch.int32))      # o_0 is the seen observation
            o1, a1 = wide[:, n:2 * n], wide[:, 3 * n:3 * n + a]
            if t == 0:
                assert done_prev is None and bool((wide[:, 3 * n:] == 0).all()) and torch.equal(o1, seen) and torch.equal(wide[:, 2 * n:3 * n], seen)
            else:
                reset = (done_prev != 0)[:, None]
                assert torch.equal(a1, torch.where(reset, torch.zeros_like(prev_act), prev_act))                      # the policy's own last action
                assert torch.equal(o1, torch.where(reset, wide[:, :n], prev_wide[:, :n]))
                want = history.reference(prev_wide.cpu().numpy(), seen.cpu().numpy(), prev_act.cpu().numpy(), done_prev.cpu().numpy(), n, a, 2, 2)
                assert np.array_equal(wide.cpu().numpy().view(np.int32), want.view(np.int32)), t
                resets += int(reset.sum())
                carried += int((~reset).sum())
            prev_wide, prev_act = wide, act
        assert resets > 0 and carried > 0, again
    player.end_sweep()


def test_a_plain_checkpoint_plays_byte_for_byte_as_the_loop_without_a_history(torch_cuda, checkpoint):
    torch = torch_cuda
    from isaacgym_amd import play
    pol = load_policy(checkpoint(TT))
    assert pol.history is None and pol.base_num_obs == pol.net.num_obs
    player = play.Player(make_plain(TT, 64, SEED), pol, games_num=100, poll_every=8, max_steps=STEPS)
    assert player._stacks == {}
    res = player.run()
    assert "history" not in res and res["games"] >= 100
    # the loop as it was before the feature, with no history object anywhere: policy on the raw observation, step, accumulate
    task = make_plain(TT, 64, SEED)
    stats = play.EpisodeStats(64, 1, 100, torch.device(DEV))
    task.reset_idx()
    stats.reset()
    pol._counter = 0
    obs = task.reset()["obs"]
    for _ in range(res["steps_played"]):
        act, _ = pol.act(obs, deterministic=True, seed=0)
        out, rew, done, _ = task.step(act)
        stats.accumulate(rew, done)
        obs = out["obs"]
    want = play.summarize(stats.read_groups()[0], 1)
    assert want == {k: res[k] for k in want} and set(res) == set(want) | {"steps_played", "seconds"}


def test_a_history_checkpoint_plays_against_a_plain_one_in_one_paired_pass(torch_cuda, history_checkpoint, checkpoint):
    from isaacgym_amd import play
    path, rec = history_checkpoint
    with_history, plain = load_policy(path), load_policy(checkpoint(TT))
    player = play.Player(make_plain(TT, 64, SEED), [with_history, plain], sweep=play.Sweep([{}, {}], paired=True), paired_diff=True, games_num=32, poll_every=8,
                         max_steps=STEPS)
    res = player.run()
    assert res["history"] == [rec, None] and len(res["groups"]) == 2 and len(res["paired_diff"]["cells"]) == 2
    assert player.policy_obs.shape == (64, rec["width"]) and player.actions.shape == (64, 7)
    assert res["paired_diff"]["cells"][0]["diff"] == 0.0                                          # the baseline against itself
    # the plain cell plays what it plays without a history policy beside it (two objects: each cell is forwarded on its own 32 rows, as above)
    alone = play.Player(make_plain(TT, 64, SEED), [load_policy(checkpoint(TT)), plain], sweep=play.Sweep([{}, {}], paired=True), paired_diff=True, games_num=32, poll_every=8,
                        max_steps=STEPS).run()
    assert "history" not in alone and res["groups"][1] == alone["groups"][1]


def test_a_policy_whose_base_width_is_not_the_tasks_is_refused(torch_cuda, history_checkpoint, checkpoint):
    torch = torch_cuda
    from isaacgym_amd import play
    from isaacgym_amd.policy import RLGamesPolicy
    path, rec = history_checkpoint
    task = make_plain(TT, 64, SEED)
    pol = load_policy(path)
    pol.base_num_obs += 1
    with pytest.raises(ValueError, match="the policy maps 81 observations to 7 actions, the task has 80 and 7"):
        play.Player(task, pol)
    pol = load_policy(path)
    pol.history = None                                         # a wide network with no record: the present refusal
    pol.base_num_obs = pol.net.num_obs
    with pytest.raises(ValueError, match="the policy maps 254 observations"):
        play.Player(task, pol)
    ck = torch.load(checkpoint(TT), map_location="cpu", weights_only=True)
    with pytest.raises(ValueError, match="history: the record .* does not describe this network"):
        RLGamesPolicy(ck["model"], DEV, history=rec)           # a plain network under a history record
