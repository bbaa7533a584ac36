"""The rollout snippet of README.md, run as written (with a synthetic rl_games-layout checkpoint): python tools/readme_snippet_check.py on the GPU box."""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, isaacgym_amd
from isaacgym_amd.policy import RLGamesPolicy
from test_policy_mlp import _rlgames_state_dict
sd = _rlgames_state_dict(torch, 313, (2048, 1536, 1024, 1024, 512, 512), 27, torch.Generator().manual_seed(0))
os.makedirs("gpurun_out", exist_ok=True)
torch.save({"model": sd}, "gpurun_out/ckpt.pth")
env = isaacgym_amd.make(task="HumanoidPingpongTiltNESSparse27DOFG1", num_envs=4096, sim_device="cuda:0", rl_device="cuda:0")
policy = RLGamesPolicy.load("gpurun_out/ckpt.pth", "cuda:0")
obs = env.reset()["obs"]
tot = 0.0
for _ in range(100):
    actions, values = policy.act(env.obs_buf, deterministic=True)
    obs, rew, done, info = env.step(actions)
    tot += float(rew.mean())
print("ok", obs["obs"].shape, float(values.mean()), tot, int(done.sum()))
# ... and the Player snippet (a synthetic checkpoint for the 7-dof task; a short episode so that 200 games finish within tens of steps)
from isaacgym_amd import scene
from isaacgym_amd.play import Player
sd = _rlgames_state_dict(torch, 80, (2048, 1536, 1024, 1024, 512, 512), 7, torch.Generator().manual_seed(0))
import tempfile
ckpt_tt = os.path.join(tempfile.mkdtemp(prefix="readme_snippet_"), "HumanoidPingpongTiltG1.pth")
torch.save({"model": sd}, ckpt_tt)
cfg = scene.default_task_cfg("TT")
cfg["env"]["episodeLength"] = 12
player = Player(isaacgym_amd.make(task="HumanoidPingpongTiltG1", num_envs=4096, cfg=cfg), RLGamesPolicy.load(ckpt_tt, "cuda:0"), games_num=200)
result = player.run()
print("ok", result["games"], result["av_reward"], result["av_steps"], result["steps_played"])
