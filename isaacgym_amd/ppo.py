"""A PPO trainer on the native env and network: rl_games' `a2c_continuous` as the reference configures it
(cfg/train/HumanoidPingpongTiltG1PPO.yaml), with the minibatch tail on the device (C ABI: include/ppenv_ppo.h).

One epoch (`PPOTrainer.train_epoch`):

    rollout      RolloutCollector: horizon x (native forward + action draw + fused env step), bootstrap value, GAE
    per epoch    value de-normalisation before GAE, old_neglogp on the stored actions, value statistics, advantage normalisation
    minibatch    forward (input statistics update) -> ppenv_ppo_loss_grad -> NativeMLPLearner.backward(d_head)
                 -> ppenv_ppo_grad_sumsq -> ppenv_ppo_adam_step -> sync_weights

There is no host synchronisation inside an epoch: the loss scale, the step count and every statistic stay on the device.

Videos while training (the reference's capture_video / RecordVideo, train.py:132-144): `PPOTrainer.set_capture(render.TrainingCapture(...))`,
`fit(..., capture=...)`, `--capture-video`.  The collector calls the capture after every control step; it launches renders into a device
ring and reads nothing, so a run with capture is bitwise the run without and an epoch still has no host synchronisation.

Semantics.  The loss terms are restated from rl_games' published a2c_continuous / common_losses (rl_games is absent offline: parity
unpinned, the same status as tools/ppo_epoch_bench.py): the clipped surrogate, the clipped value loss, the soft bound loss at +-1.1, and
loss = mean(a) + 0.5 critic_coef mean(c) - entropy_coef entropy + bounds_loss_coef mean(b).  The gradient-norm clip is
clip_grad_norm_'s, the optimizer torch.optim.Adam's, the loss scale torch GradScaler's (init 65536, x0.5 and a skipped step on a
non-finite gradient, x2 after 2000 clean steps) — with two bounds GradScaler does not have: never below 1.0, never grown to inf (DeviceAdam).

Deviations from rl_games:
  - rl_games stores the unclamped action draw; the collector stores the CLAMPED actions the env consumed.  The ratio is evaluated on the
    clamped actions, and old_neglogp is re-evaluated on them under the rollout's mu / sigma once per epoch (as tools/ppo_epoch_bench.py
    does), so that the ratio starts at 1.
  - `value_bootstrap` is a no-op here: `time_outs` is identically false for these tasks (vec_task.py, step), so there is nothing to add
    to the rewards.
  - The minibatches are the contiguous row ranges of the horizon-major buffers, in order.
  - Privileged critic inputs (critic_inputs=, below) are this project's own specification.  rl_games' central value
    (`central_value_config`) is a SEPARATE network with its own optimizer, statistics and minibatches, fed VecTask's `states`; here the
    critic tower of the one network reads extra first-layer columns, and loss, optimizer, schedule and minibatches are the ones above.

Checkpoints are rl_games' layout: {"model": network + value_mean_std.*, "epoch", "frame", "optimizer"}; RLGamesPolicy.load serves them.
They also carry "history" (the record of an observation and action history, below), "meter" (the score meter's struct), "last_mean_rewards" (the best score so far) and "latency" (the two delay ranges the
run trained under, {"action_delay": [lo, hi], "obs_delay": [lo, hi]}: a record — load() accepts files without any of them, and the
trainer that loads keeps the delays it was built with).

Control latency (PPOTrainer(action_delay=, obs_delay=), --action-delay / --obs-delay K | LO:HI): the rollout runs with a delay line on the
command path and / or the sensing path, fixed or drawn per env at every episode start (RolloutCollector; include/ppenv_train_delay.h;
DESIGN §5d "Training under latency").  Off by default, and then nothing is built.

Domain randomisation (PPOTrainer(randomization=, adr=), --randomize / --adr TABLE=...): a reset-time plan (include/ppenv_dr.h) or automatic
domain randomisation, a device-resident curriculum over the tables' ranges (adr.AutoRandomizer; include/ppenv_dr_adr.h), run from the
collector's per-step hook (DESIGN §5d "Randomisation and ADR in training").  Off by default, and then nothing is built.

Sensor noise and dropouts (PPOTrainer(obs_noise=, obs_drop=, action_noise=, action_drop=, sensor_columns=), --obs-noise / --obs-drop / --action-noise /
--action-drop S | LO:HI, --obs-noise-columns / --obs-drop-columns / --action-noise-columns / --action-drop-columns SPEC): the rollout runs with a sensor
line on the sensing path and one on the command path (sensor.SensorLine; include/ppenv_sensor.h holds the rule; DESIGN §5e "Sensor noise and
dropouts").  Off by default, and then nothing is built.

Privileged critic inputs (PPOTrainer(critic_inputs=("tables", "latency", "raw_obs")), --critic-inputs tables,latency,raw_obs): an asymmetric
actor-critic.  The named quantities — the env's randomisation tables, its delays, its undelayed observation — are gathered per control step
into `col.priv` (critic_input.CriticInput; include/ppenv_critic_input.h) and feed first-layer columns that only the critic's weights read;
the actor's weights over them are exactly zero and never reach the optimizer (policy.NativeMLP(num_priv=); DESIGN §5d "Privileged critic
inputs").  The columns have running statistics of their own (`critic_mean_std.*` in the checkpoint's model), updated under the rule of the
observation statistics.  Checkpoints carry the record under "critic_inputs" (names, columns per name, P); load() refuses a file whose P or
names differ.  RLGamesPolicy serves such a checkpoint's actor as it stands.  Off by default, and then nothing is built.

Observation and action history (PPOTrainer(history=(Ho, Ha)), --obs-history Ho --action-history Ha): the network's input rows become the
observation the policy sees now, the Ho it saw before and its own last Ha actions, stacked on the device (history.HistoryStack;
include/ppenv_history.h; DESIGN §5d "Observation and action history").  Off by default, and then nothing is built.

The score (GameMeter; C ABI: include/ppenv_ppo_meter.h) is rl_games' game_rewards / game_lengths: AverageMeter(games_to_track) over the
finished games' unscaled returns (agent 0's row of each env) and lengths, updated once per epoch over the collector's horizon by two
launches.  `fit` is rl_games' loop around train_epoch(): the periodic save to nn/<name>.pth, the best checkpoint from save_best_after on,
the stop on score_to_win (yaml:63-66).  Two deviations: the meter is fp64 with a fixed summation order (rl_games: fp32 torch), and the
best checkpoint goes to nn/<name>_best.pth while nn/<name>.pth keeps meaning "latest" (rl_games: best in <name>.pth, latest in last_...).

Data-parallel training (the reference's multi_gpu mode: `torchrun --nproc_per_node=N train.py multi_gpu=True`; rl_games' multi-GPU a2c).  Each
rank owns an env shard (isaacgym_amd.make(multi_gpu=True)) and a learner; `PPOTrainer(..., group=...)` switches it on when the group has more
than one rank (or with force=True: RCCL with one rank).  Restated from rl_games' published code like the rest of this module (absent offline:
parity unpinned):
  - at the start rank 0's parameters, log-std and input / value statistics are broadcast (rl_games broadcasts its model state_dict);
  - every minibatch step all-reduces the gradients (one collective per layer beside the backward, distributed.GradientBuckets; the log-std
    gradient lives right after the heads' gradients and travels in their collective) and steps on their rank mean, formed inside the Adam kernel (DeviceAdam(world=...): rl_games' all_grads / world_size);
    all ranks see the same summed bits, so parameters, moments and the loss scale stay identical, and a non-finite sum skips the step on all;
  - per rank, as in rl_games: the input and value statistics (updated from the rank's own shard, never synchronised), advantage
    normalisation, minibatch_size;
  - global: the epoch statistics of train_epoch() (loss terms, KL and clip fraction averaged over the ranks; episode sums and counts summed),
    in one all-reduce per epoch, and `frame` (horizon x rows x world).
  - the score meter is per rank, as in rl_games; train_epoch() returns rank 0's (one 40-byte broadcast per epoch), so every rank takes fit's
    decisions from the same numbers and all leave the loop in the same epoch.
Only rank 0 writes checkpoints; load() on every rank reads the same file, so the ranks resume identical — all with rank 0's statistics.
"""
import argparse
import ctypes as C
import dataclasses
import json
import math
import os
import time

import numpy as np
import torch

from . import _lib, cfgyaml, scene
from . import adr as adr_mod
from . import critic_input as critic_input_mod
from . import curriculum as curriculum_mod
from . import distributed as D
from . import history as history_mod
from ._lib import PPOAdam, PPOLossArgs, PPOMeter, PPOTensor     # the ctypes mirrors of include/ppenv_ppo.h and ppenv_ppo_meter.h (bound in _lib.load)
from .collector import RolloutCollector, gae
from .latency import delay_range, latency_text
from . import sensor as sensor_mod
from .policy import UNITS, NativeActorCritic, RunningMeanStd, layers_from_rlgames_state_dict, sampler_stream_seed

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
STATS = ("loss", "a_loss", "c_loss", "b_loss", "entropy", "kl", "clip_frac")     # ppenv_ppo_loss_grad's stats[] (include/ppenv_ppo.h)
SOFT_BOUND = 1.1                          # rl_games a2c_continuous.bound_loss
OPT_PARTS = 512                           # workgroups of the optimizer launches: two per CU
NO_SCORE = -100500.0                      # rl_games a2c_common: last_mean_rewards before any best checkpoint


# ---- configuration ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PPOConfig:
    """rl_games' a2c_continuous settings.  Defaults: cfg/train/HumanoidPingpongTiltG1PPO.yaml (the 27-dof task has no train yaml of its own and
    uses them too), except minibatch_size, whose yaml value 4 (line 74, commented "# 8192") is not a usable minibatch."""
    gamma: float = 0.99                   # yaml:58
    tau: float = 0.95                     # yaml:59
    learning_rate: float = 2e-5           # yaml:60
    lr_schedule: str = "constant"         # yaml:61
    e_clip: float = 0.2                   # yaml:72
    critic_coef: float = 4.0              # yaml:76
    clip_value: bool = True               # yaml:77
    bounds_loss_coef: float = 1e-4        # yaml:79
    entropy_coef: float = 0.0             # yaml:69
    grad_norm: float = 10.0               # yaml:68
    truncate_grads: bool = True           # yaml:70
    normalize_advantage: bool = True      # yaml:57
    normalize_input: bool = True          # yaml:51
    normalize_value: bool = True          # yaml:52
    mixed_precision: bool = True          # yaml:50
    horizon_length: int = 32              # yaml:73
    mini_epochs: int = 5                  # yaml:75
    minibatch_size: int = 8192            # yaml:74 "# 8192"
    reward_scale: float = 0.01            # yaml:55-56 reward_shaper.scale_value
    sigma_init: float = -2.0              # yaml:20-22 sigma_init const_initializer val
    fixed_sigma: bool = True              # yaml:23
    max_epochs: int = 200000              # yaml:64
    save_frequency: int = 1500            # yaml:66
    score_to_win: float = 20000.0         # yaml:63
    save_best_after: int = 3000           # yaml:65
    games_to_track: int = 100             # rl_games a2c_common default (the yaml does not set it): the score meter's window
    units: tuple = tuple(UNITS)           # yaml:29
    # GradScaler (torch.cuda.amp defaults; rl_games builds it with enabled=mixed_precision)
    init_scale: float = 65536.0
    growth_interval: int = 2000

    KEYS = {                              # PPOConfig field <- params.config key
        "gamma": "gamma", "tau": "tau", "learning_rate": "learning_rate", "lr_schedule": "lr_schedule", "e_clip": "e_clip",
        "critic_coef": "critic_coef", "clip_value": "clip_value", "bounds_loss_coef": "bounds_loss_coef", "entropy_coef": "entropy_coef",
        "grad_norm": "grad_norm", "truncate_grads": "truncate_grads", "normalize_advantage": "normalize_advantage",
        "normalize_input": "normalize_input", "normalize_value": "normalize_value", "mixed_precision": "mixed_precision",
        "horizon_length": "horizon_length", "mini_epochs": "mini_epochs", "minibatch_size": "minibatch_size", "max_epochs": "max_epochs",
        "save_frequency": "save_frequency", "score_to_win": "score_to_win", "save_best_after": "save_best_after",
        "games_to_track": "games_to_track"}

    @classmethod
    def from_train_cfg(cls, train, task_cfg=None, **overrides):
        """cfg["train"] (a composed train yaml: `params.config`, `params.network`) -> PPOConfig; `overrides` (field=value) win over the yaml.
        task_cfg: cfg["task"], checked for `randomize`.  Raises ValueError naming the key for what the trainer does not run."""
        params = train["params"] if "params" in train else train
        c, net = params.get("config", {}), params.get("network", {})
        kw = {}
        for field, key in cls.KEYS.items():
            if key in c and c[key] not in ("", None):
                kw[field] = c[key]
        if "reward_shaper" in c and "scale_value" in c["reward_shaper"]:
            kw["reward_scale"] = c["reward_shaper"]["scale_value"]
        cont = net.get("space", {}).get("continuous", {})
        if "sigma_init" in cont and "val" in cont["sigma_init"]:
            kw["sigma_init"] = cont["sigma_init"]["val"]
        if "fixed_sigma" in cont:
            kw["fixed_sigma"] = cont["fixed_sigma"]
        if "units" in net.get("mlp", {}):
            kw["units"] = tuple(net["mlp"]["units"])
        kw.update(overrides)
        types = {f.name: f.type for f in dataclasses.fields(cls)}
        for k, v in list(kw.items()):
            t = types[k]
            if t in (float, "float"):
                kw[k] = float(v)              # learning_rate: 2e-5 arrives as the string "2e-5" from YAML 1.1
            elif t in (int, "int"):
                kw[k] = int(v)
            elif t in (bool, "bool"):
                kw[k] = v if isinstance(v, bool) else str(v).lower() == "true"
        cfg = cls(**kw)
        cfg.check()
        if task_cfg is not None and bool(task_cfg.get("task", {}).get("randomize", False)):
            raise ValueError("task.randomize: True is not supported by PPOTrainer: it drives the native env below VecTask.step's randomisation "
                             "hook; set task.randomize=False")
        return cfg

    def check(self, rows=None):
        """The settings this trainer runs; rows: actor rows of the env (num_envs x num_agents), for the minibatch's divisibility."""
        mb = self.minibatch_size
        hint = "; use minibatch_size=8192 (the yaml's comment) or 32768"
        if mb <= 0 or mb % 64:
            raise ValueError(f"minibatch_size: {mb} is not a positive multiple of 64 (the learner's row tile){hint}")
        if rows is not None and (self.horizon_length * rows) % mb:
            raise ValueError(f"minibatch_size: {mb} does not divide horizon_length x rows = {self.horizon_length} x {rows}{hint}")
        if self.lr_schedule != "constant":
            raise ValueError(f"lr_schedule: {self.lr_schedule!r} is not supported (only 'constant', every reference yaml's value)")
        if not self.fixed_sigma:
            raise ValueError("fixed_sigma: False is not supported (the network has a learnable, observation-independent log-std)")
        if tuple(self.units) != tuple(UNITS):
            raise ValueError(f"units: {list(self.units)} — the native network is built for {UNITS}")
        if self.games_to_track < 1:
            raise ValueError(f"games_to_track: {self.games_to_track} is not a positive number of games (rl_games' default is 100)")


# ---- the loss gradient in fp64: what ppenv_ppo_loss_grad computes ------------------------------------------------------------------
def loss_grad_reference(mu, value, actions, old_neglogp, old_mu, old_sigma, advantages, old_values, returns, logstd, e_clip=0.2, critic_coef=4.0,
                        bounds_loss_coef=1e-4, entropy_coef=0.0, clip_value=True, scale=1.0, soft_bound=SOFT_BOUND):
    """numpy fp64, per-row analytic gradient of rl_games' a2c_continuous loss (the kernel's formulas).  mu / actions / old_mu [M, A],
    value / old_neglogp / advantages / old_values / returns [M], old_sigma / logstd [A] -> dict(d_mu [M, A], d_value [M], d_logstd [A]: all
    d(loss x scale); and the unscaled statistics named in STATS)."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    mu, value, act, onlp, omu, osg = f(mu), f(value).reshape(-1), f(actions), f(old_neglogp), f(old_mu), f(old_sigma)
    adv, ov, ret, ls = f(advantages), f(old_values), f(returns), f(logstd)
    m, a = mu.shape
    sg = np.exp(ls)
    z = (act - mu) / sg
    nlp = 0.5 * (z * z).sum(1) + HALF_LOG_2PI * a + ls.sum()
    ratio = np.exp(onlp - nlp)
    s1, s2 = -adv * ratio, -adv * np.clip(ratio, 1.0 - e_clip, 1.0 + e_clip)
    a_loss = np.maximum(s1, s2)
    g = np.where(s1 >= s2, adv * ratio, 0.0)                 # d a_loss / d nlp
    cu = (value - ret) ** 2
    if clip_value:
        d = value - ov
        vc = ov + np.clip(d, -e_clip, e_clip)
        cc = (vc - ret) ** 2
        c_loss = np.maximum(cu, cc)
        dv = np.where(cu >= cc, 2.0 * (value - ret), np.where(np.abs(d) <= e_clip, 2.0 * (vc - ret), 0.0))
    else:
        c_loss, dv = cu, 2.0 * (value - ret)
    hi, lo = np.maximum(mu - soft_bound, 0.0), np.minimum(mu + soft_bound, 0.0)
    b_loss = (hi * hi + lo * lo).sum(1)
    entropy = (0.5 + HALF_LOG_2PI + ls).sum()
    kl = (np.log(osg / sg + 1e-5) + (sg * sg + (omu - mu) ** 2) / (2.0 * (osg * osg + 1e-5)) - 0.5).sum(1)
    gs = scale / m
    d_mu = gs * (-g[:, None] * z / sg + bounds_loss_coef * (2.0 * hi + 2.0 * lo))
    d_value = gs * 0.5 * critic_coef * dv
    d_logstd = gs * (g[:, None] * (1.0 - z * z)).sum(0) - scale * entropy_coef
    loss = a_loss.mean() + 0.5 * critic_coef * c_loss.mean() - entropy_coef * entropy + bounds_loss_coef * b_loss.mean()
    return dict(d_mu=d_mu, d_value=d_value, d_logstd=d_logstd, loss=loss, a_loss=a_loss.mean(), c_loss=c_loss.mean(), b_loss=b_loss.mean(),
                entropy=entropy, kl=kl.mean(), clip_frac=(np.abs(ratio - 1.0) > e_clip).mean())


# ---- the device kernels on torch tensors ------------------------------------------------------------------------------------------
class LossGrad:
    """ppenv_ppo_loss_grad for minibatches of up to `max_rows` rows: `d_head` [rows, A + 1] (what NativeMLPLearner.backward takes),
    `d_logstd` [A] (the caller's buffer when given), and one row of STATS per call into the caller's `stats` row."""

    def __init__(self, num_actions, max_rows, device, cfg, d_logstd=None):
        self.a, self.cfg = int(num_actions), cfg
        assert 0 < self.a <= 32, "one lane per row holds the row's actions: at most 32"
        dev = torch.device(device)
        self.d_head = torch.zeros((max_rows, self.a + 1), dtype=torch.float32, device=dev)
        self.d_logstd = torch.zeros(self.a, dtype=torch.float32, device=dev) if d_logstd is None else d_logstd     # the optimizer's gradient buffer
        self.partial = torch.zeros(int(_lib.lib().ppenv_ppo_loss_partial_floats(max_rows)), dtype=torch.float32, device=dev)

    def __call__(self, mu, value, actions, old_mu, old_sigma, old_neglogp, advantages, old_values, returns, logstd, scale, stats):
        """mu / actions / old_mu [M, >= A] fp32 with unit column stride (any row stride); value [M, 1] (any row stride); old_sigma / logstd [A];
        old_neglogp / advantages / old_values / returns [M] contiguous; scale: a device fp32 scalar; stats: fp32 [8] -> d_head[:M]."""
        m, c = mu.shape[0], self.cfg
        for t in (mu, value, actions, old_mu):
            assert t.dtype == torch.float32 and t.stride(1) == 1 and t.shape[0] == m
        for t in (old_neglogp, advantages, old_values, returns, old_sigma, logstd, scale, stats):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert m <= self.d_head.shape[0] and old_neglogp.numel() == advantages.numel() == old_values.numel() == returns.numel() == m
        p = PPOLossArgs(m, self.a, mu.data_ptr(), mu.stride(0), value.data_ptr(), value.stride(0), actions.data_ptr(), actions.stride(0),
                        old_mu.data_ptr(), old_mu.stride(0), old_sigma.data_ptr(), old_neglogp.data_ptr(), advantages.data_ptr(),
                        old_values.data_ptr(), returns.data_ptr(), logstd.data_ptr(), c.e_clip, c.critic_coef, c.bounds_loss_coef, SOFT_BOUND,
                        c.entropy_coef, int(c.clip_value), scale.data_ptr(), self.d_head.data_ptr(), self.d_head.stride(0),
                        self.d_logstd.data_ptr(), stats.data_ptr(), self.partial.data_ptr())
        _lib.check(_lib.lib().ppenv_ppo_loss_grad(C.byref(p), _lib.stream(mu)))
        return self.d_head[:m]


def _matrix(t):
    """(rows, cols, row stride) of a tensor whose rows are evenly strided and whose last dimension is contiguous."""
    if t.dim() == 1:
        assert t.stride(0) == 1
        return 1, t.shape[0], t.shape[0]
    assert t.stride(-1) == 1
    for d in range(t.dim() - 2):
        assert t.stride(d) == t.shape[d + 1] * t.stride(d + 1), "rows must be evenly strided"
    return int(np.prod(t.shape[:-1])), t.shape[-1], t.stride(-2)


class DeviceAdam:
    """clip_grad_norm_ + torch.optim.Adam + GradScaler on the device, over `params` / `grads` as they are (any evenly strided rows).
    Two launches per step (ppenv_ppo_grad_sumsq, ppenv_ppo_adam_step).  `scale` is the device scalar the loss gradient multiplies by;
    the scaler state (include/ppenv_ppo.h ppenv_ppo_scaler) is double-buffered in `state` [2, 8] int32: the step reads row `cur`, writes
    row 1 - cur, and `cur` flips on the host (the host never reads the state).
    The scale is bounded — a deliberate departure from torch's GradScaler, which bounds neither end (include/ppenv_ppo.h): with dynamic=True
    it never leaves a step below 1.0 (the scale of dynamic=False; a state loaded from below, load_state_dict included, is lifted by its next
    step), it does not grow where scale x 2 is not finite, and a step at a scale that is not a normal positive number is skipped, so finite
    gradients never write a non-finite parameter.  fields()["floor_hits"] counts the steps in which the floor held the scale.
    world: data-parallel ranks.  Above 1, `grads` hold the all-reduced SUMS over the ranks (distributed.GradientBuckets(mean=False)) and the
    kernels step on their rank means fl(g / world); 0 or 1: one rank, bit-identical to the default."""

    def __init__(self, params, grads, lr, max_norm=10.0, truncate=True, init_scale=65536.0, growth_interval=2000, dynamic=True,
                 betas=(0.9, 0.999), eps=1e-8, parts=OPT_PARTS, world=1):
        assert len(params) == len(grads) and 0 < len(params) <= 64
        self.params, self.grads = list(params), list(grads)
        dev = self.device = self.params[0].device
        self.exp_avg = [torch.zeros(p.shape, dtype=torch.float32, device=dev) for p in self.params]
        self.exp_avg_sq = [torch.zeros(p.shape, dtype=torch.float32, device=dev) for p in self.params]
        items = []
        for p, g, m, v in zip(self.params, self.grads, self.exp_avg, self.exp_avg_sq):
            assert p.dtype == g.dtype == torch.float32 and p.shape == g.shape and p.device == g.device == dev
            rows, cols, ld_p = _matrix(p)
            _, _, ld_g = _matrix(g)
            items.append(PPOTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), rows, cols, ld_p, ld_g))
        arr = (PPOTensor * len(items))(*items)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)        # copied once
        self.count, self.parts = len(items), int(parts)
        self.slab = torch.zeros(self.parts, dtype=torch.float64, device=dev)
        self.lr = torch.full((), float(lr), dtype=torch.float32, device=dev)
        if int(world) < 0:
            raise ValueError(f"world: {world} ranks")
        self.hp = PPOAdam(betas[0], betas[1], eps, max_norm, int(truncate), 2.0 if dynamic else 1.0, 0.5 if dynamic else 1.0, int(growth_interval),
                          int(world))
        self.state = torch.zeros((2, 8), dtype=torch.int32, device=dev)
        self.state[:, 0:1].view(torch.float32).fill_(float(init_scale))
        self.cur = 0

    @property
    def scale(self):
        """The current loss scale: a device fp32 scalar view (the loss gradient reads it; changes in place after every step)."""
        return self.state[self.cur, 0:1].view(torch.float32)

    def fields(self):
        """The current state as 0-dim device tensors: scale, growth_tracker, step, skipped, grad_norm, floor_hits."""
        s = self.state[self.cur]
        return dict(scale=s[0:1].view(torch.float32)[0], growth_tracker=s[1], step=s[2], skipped=s[3], grad_norm=s[4:5].view(torch.float32)[0],
                    floor_hits=s[5])

    def step(self):
        L = _lib.lib()
        st = _lib.stream(self.slab)
        _lib.check(L.ppenv_ppo_grad_sumsq(self.table.data_ptr(), self.count, self.slab.data_ptr(), self.parts, st))
        _lib.check(L.ppenv_ppo_adam_step(self.table.data_ptr(), self.count, self.slab.data_ptr(), self.parts, self.hp, self.lr.data_ptr(),
                                         self.state[self.cur].data_ptr(), self.state[1 - self.cur].data_ptr(), st))
        self.cur = 1 - self.cur

    def state_dict(self):
        return {"exp_avg": [t.detach().clone() for t in self.exp_avg], "exp_avg_sq": [t.detach().clone() for t in self.exp_avg_sq],
                "scaler": self.state[self.cur].detach().clone(), "lr": self.lr.detach().clone()}

    def load_state_dict(self, sd):
        with torch.no_grad():
            for dst, src in zip(self.exp_avg + self.exp_avg_sq, list(sd["exp_avg"]) + list(sd["exp_avg_sq"])):
                dst.copy_(src)
            self.cur = 0
            self.state[0].copy_(sd["scaler"])
            self.state[1].copy_(sd["scaler"])
            self.lr.copy_(sd["lr"])


class GameMeter:
    """rl_games' game_rewards / game_lengths (AverageMeter(games_to_track)) on the device: ppo_meter_update (include/ppenv_ppo_meter.h) on
    torch tensors.  `cur_reward` [num_envs] f32 and `cur_len` [num_envs] i32 are the envs' running games (agent 0's row of each env), the
    meter struct holds the two running means, the games they stand for, and the counts.  Nothing here reads the device on the host."""

    def __init__(self, num_envs, num_agents, games_to_track, device):
        self.num_envs, self.num_agents, self.games_to_track = int(num_envs), int(num_agents), int(games_to_track)
        if self.num_envs < 1 or self.num_agents not in (1, 2) or self.games_to_track < 1:
            raise ValueError(f"GameMeter: num_envs {num_envs} (>= 1), num_agents {num_agents} (1 or 2), games_to_track {games_to_track} (>= 1)")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:                       # tensors carry an index: compare like with like
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.rows = self.num_envs * self.num_agents
        self.L = _lib.lib()
        self.cur_reward = torch.zeros(self.num_envs, dtype=torch.float32, device=dev)
        self.cur_len = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)
        self._meter = torch.zeros(C.sizeof(PPOMeter), dtype=torch.uint8, device=dev)           # all zero: the empty meter
        self._partial = torch.zeros(0, dtype=torch.uint8, device=dev)                          # grows to the longest horizon seen

    def update(self, rewards, dones):
        """One horizon: rewards [H, rows] f32 (unscaled), dones [H, rows] int64 — RolloutCollector's buffers or row-strided views of larger
        ones (unit stride inside a row), on this device.  Two launches, no synchronisation."""
        if rewards.dim() != 2 or rewards.shape != dones.shape or rewards.shape[0] < 1 or rewards.shape[1] != self.rows or \
                rewards.dtype != torch.float32 or dones.dtype != torch.int64 or rewards.device != self.device or dones.device != self.device or \
                (self.rows > 1 and (rewards.stride(1) != 1 or dones.stride(1) != 1)):
            raise ValueError(f"GameMeter.update: rewards must be float32 and dones int64, [H, {self.rows}] with unit stride inside a row, on {self.device}")
        h = rewards.shape[0]
        ld_r, ld_d = (rewards.stride(0), dones.stride(0)) if h > 1 else (self.rows, self.rows)
        need = int(self.L.ppo_meter_partial_bytes(h, self.num_envs))
        if self._partial.numel() < need:
            self._partial = torch.zeros(need, dtype=torch.uint8, device=self.device)
        _lib.check(self.L.ppo_meter_update(rewards.data_ptr(), ld_r, dones.data_ptr(), ld_d, h, self.num_envs, self.num_agents, self.games_to_track,
                                           self.cur_reward.data_ptr(), self.cur_len.data_ptr(), self._meter.data_ptr(), self._partial.data_ptr(),
                                           _lib.stream(self.device)), self.L)

    def snapshot(self):
        """One copy of the meter struct as it stands at this point of the stream (uint8 [sizeof ppenv_ppo_meter]); fields(snapshot) names it."""
        return self._meter.clone()

    def fields(self, raw=None):
        """The meter as 0-dim device tensors: mean_reward, mean_length (fp64), current_size, games_total, updates (int64).  Views of the
        live struct, which change in place with every update — or of `raw`, a snapshot()."""
        o, raw = PPOMeter, self._meter if raw is None else raw
        means, counts = raw[:o.current_size.offset].view(torch.float64), raw[o.current_size.offset:].view(torch.int64)
        return dict(mean_reward=means[0], mean_length=means[1], current_size=counts[0], games_total=counts[1], updates=counts[2])

    def state_dict(self):
        """The meter struct only: the envs' running games restart at zero on resume, as the envs themselves do."""
        return {"meter": self._meter.detach().clone()}

    def load_state_dict(self, sd):
        with torch.no_grad():
            self._meter.copy_(sd["meter"])
            self.cur_reward.zero_()
            self.cur_len.zero_()

    def state_bytes(self):
        """cur_reward, cur_len and the meter struct as host bytes (the tests compare them)."""
        return self.cur_reward.cpu().numpy().tobytes(), self.cur_len.cpu().numpy().tobytes(), self._meter.cpu().numpy().tobytes()


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
def _denorm_(x, rms):
    """rl_games RunningMeanStd(unnorm=True) in place: clamp(+-5), then x sqrt(var + eps) + mean."""
    return x.clamp_(-5.0, 5.0).div_(rms.inv_std).add_(rms.mean)


def _norm(x, rms):
    return ((x - rms.mean) * rms.inv_std).clamp_(-5.0, 5.0)


class PPOTrainer:
    """rl_games' a2c_continuous on a task built by isaacgym_amd.make(...): its native handle (task.env: PPEnv or TAEnv) runs under
    RolloutCollector; the network is NativeActorCritic (nn.Linear's default initialisation, rl_games' `initializer: default`) with a learnable
    fixed log-std (its `sigma` parameter, initialised to sigma_init) and, with normalize_value, a value RunningMeanStd of width 1.
    group: a torch.distributed process group (None: the default group, if one is initialised); data-parallel when it has more than one rank, or
    with force=True (the collectives with one rank, as bench.py --force-dist).  See the module docstring for what is per rank and what is global.
    outcomes: the 27-dof task's five head-counts (task.enable_outcomes(); the other tasks raise ValueError) — train_epoch() then also returns
    outcome_windows, outcome_envs and the five outcome_<name> rates of the most recent window.  The step kernel's clear sums them into a struct
    of their own: parameters, moments, scaler, statistics and meter stay bitwise those of a run without.  Not checkpointed: the envs restart on
    resume.
    action_delay, obs_delay: train under control latency — whole control steps, an int K (every env, always) or a (lo, hi) pair drawn anew
    per env at every episode start (RolloutCollector; include/ppenv_train_delay.h — this build's own rule, the reference delays nothing).
    The env consumes the command of that many steps ago and the policy sees — and the learner trains on — the observation of that many
    steps ago; the stored actions are the policy's own.  The draws are keyed scene.stream_seed(seed, scene.STREAM_LATENCY) and the task's
    env_id_offset, so ranks under seed + r share none.  Rewards, dones, GAE, the score meter, outcomes and capture are untouched; with both
    delays 0 (the default) no line is built and the run is bitwise the run without the arguments.  A fixed delay K trains under exactly
    what `python -m isaacgym_amd.play --sweep action_delay=...` measures.  Checkpoints carry the two ranges under "latency"; the lines'
    state is not checkpointed (the envs restart on resume).
    obs_noise, action_noise (an amplitude S >= 0, or a (lo, hi) range), obs_drop, action_drop (a probability 0 .. 1, or a range): train under
    sensor noise and sample dropouts (RolloutCollector; include/ppenv_sensor.h — this build's own rule, the reference adds no such noise).
    A range is drawn anew per env at every episode start, on the device.  sensor_columns: dict(obs_noise_columns=, obs_drop_columns=,
    action_noise_columns=, action_drop_columns=) of column specs ("ball_pos=1,ball_vel=4,60:67=0.5"; sensor.columns).  The sensing line
    comes before the observation delay and the history, the command line after the action delay; the policy sees — and the learner trains
    on — the noised observation, the env consumes the noised command, the stored actions are the policy's own and the `raw_obs` critic
    input stays the clean observation.  The draws are keyed scene.stream_seed(seed, scene.STREAM_SENSOR) and the task's env_id_offset, so
    data-parallel shards reproduce one handle's rows and ranks under seed + r share none.  sensor() returns the record, checkpoints carry
    it under "sensor" (a record, like "latency": load() accepts files without it and play does not read it).  With every value zero (the
    default) nothing is allocated or launched and the run is bitwise the run without the arguments.  A fixed level trains under exactly
    what `python -m isaacgym_amd.play --sweep obs_noise=...` measures.
    serve_plan, serve_paired: train on a serve plan (include/ppenv_serve.h) — cells of serve ranges over equal env groups, as
    env.set_serve_plan takes them — keyed scene.stream_seed(seed, scene.STREAM_SERVES) and the task's env_id_offset, so ranks under seed + r
    share no serves.  The collector runs the plan's launch after every env step.  A task that arrives with a plan set (task.set_serve_plan)
    is refused, as before: that plan is keyed by the task's seed, not the trainer's; clear it and pass its cells here.  One cell of pinned values trains on exactly what `python -m isaacgym_amd.play --sweep serve_speed=...` measures.
    curriculum: dict(bins=..., power=1, mix=0.25, alpha=0.3) — an adaptive serve curriculum kept on the device (include/
    ppenv_serve_curric.h — this build's own rule, the reference has none): `bins` are cell dicts (curriculum.grid(...)); every finished
    game's return (agent 0's, unscaled) is credited to the bin its ball was drawn from, and every env's next serve is drawn from a table
    that favours the bins with the lowest mean return.  One launch per control step, a fold and an update per epoch, no host read;
    data-parallel, the horizon's per-bin totals are summed over the ranks (one int64 all-reduce of 3 B words), so every rank holds the same
    table.  train_epoch() then also returns curriculum_games, curriculum_mean and curriculum_prob, [B] device tensors.  power=0 or mix=1
    keeps the statistics over uniform bins: the control run.  Checkpoints carry the plan's cells under "serve" and the curriculum's bins,
    parameters and table under "curriculum"; load() restores the table and raises ValueError on other bins.  Per-env state is not
    checkpointed.  A plan together with a curriculum is a ValueError; with neither, nothing is allocated or launched and the run is
    bitwise the run without the arguments.  clear_serve() gives the built-in serves back.
    randomization: train under reset-time domain randomisation (include/ppenv_dr.h, all of its vocabulary) — a plan dict as
    scene.reset_randomization_plan returns, or True for the actor parameters of the task cfg's own randomization_params — set on the env with
    env.set_reset_randomization, keyed scene.stream_seed(seed, scene.STREAM_TABLES) and the task's env_id_offset.  The tables are drawn once
    when the trainer is built; from then on the collector runs the plan's launch after every env step on the row of dones that step wrote,
    so an env's columns change exactly when it resets.  Noise amplitudes and gravity stay what the env has.
    adr: dict(dims=..., boundary_frac=0.25, min_games=256, t_low=..., t_high=...) — automatic domain randomisation (adr.AutoRandomizer;
    include/ppenv_dr_adr.h — this build's own rule): a current range per table, a share of the envs pinned to a boundary for a whole game,
    every boundary moved outward or back in once per epoch by the mean return of its games.  One launch per control step, a fold and an
    update per epoch, no host read; data-parallel, the per-slot totals are summed over the ranks (one int64 all-reduce of 3 S words), so
    every rank holds the same ranges.  train_epoch() then also returns adr_lo, adr_hi [D] and adr_games, adr_mean [S].  boundary_frac=0
    is fixed-range randomisation by the same kernel: the control run.  Checkpoints carry the plan under "randomization" and the
    randomizer's dims, parameters, ranges and per-slot state under "adr"; load() restores the latter and raises ValueError on other dims.
    Both arguments together are a ValueError; a task that arrives with randomize: True is refused as before; with neither, nothing is
    allocated or launched.  clear_randomization() drops both.
    critic_inputs: a tuple of critic_input.NAMES ("tables", "latency", "raw_obs"), or the CLI's comma-separated text — privileged critic
    inputs (the module docstring; this build's own rule).  `tables` needs randomization= or adr=, `latency` a delay above 0, `raw_obs` an
    obs_delay above 0: otherwise a ValueError naming the argument.  The network is then built with num_priv = P, the collector keeps
    `col.priv` [H + 1, rows, P], minibatch_step() slices it like `obs` (prepare() reads neither), and data-parallel the privileged statistics are broadcast
    with the others at the start.  critic_inputs() returns the record.  Empty (the default): the trainer is bitwise the trainer without the
    argument and `col.priv` is None.  clear_randomization() leaves the tables' columns reading the dropped tensors as they last stood.
    history: an observation and action history as the policy's input — (Ho, Ha), dict(obs=Ho, actions=Ha) or the CLI's text (history.parse;
    include/ppenv_history.h — this build's own rule): the network's rows become the observation the policy sees now, the Ho it saw before and
    its own last Ha clamped actions, W = (Ho + 1) * n + Ha * A columns, built on the device by one more launch per control step
    (RolloutCollector(history=)).  Actor and critic are both built with num_obs = W — `num_obs` is then W, `base_num_obs` the env's n —, the
    input statistics are W wide, privileged columns start at W and a `raw_obs` critic input keeps width n.  history() returns the record,
    checkpoints carry it under "history", load() refuses a file whose record differs, and RLGamesPolicy / Player serve such a checkpoint
    with a stack of their own.  Data-parallel training needs nothing new.  None (the default): the trainer is bitwise the trainer without
    the argument."""

    def __init__(self, task, cfg=None, seed=0, group=None, force=False, outcomes=False, action_delay=0, obs_delay=0, serve_plan=None, serve_paired=False,
                 curriculum=None, randomization=None, adr=None, critic_inputs=(), history=None, obs_noise=0.0, obs_drop=0.0, action_noise=0.0, action_drop=0.0,
                 sensor_columns=None):
        self.cfg = cfg = PPOConfig() if cfg is None else cfg
        critic_inputs = critic_input_mod.parse(critic_inputs)
        if task.randomize:
            raise ValueError("task.randomize: True is not supported by PPOTrainer: it drives the native env below VecTask.step's randomisation hook")
        if randomization is not None and randomization is not False and adr is not None:
            raise ValueError("randomization together with adr: a reset-time plan and ADR write the same randomisation tables")
        if task._serve_plan is not None:
            raise ValueError("a task with a serve plan set is not supported by PPOTrainer: the collector drives the env below VecTask.step, so the plan's "
                             "per-step launch would not run; call task.clear_serve_plan() first and pass the cells as serve_plan=")
        if curriculum is not None and serve_plan is not None:
            raise ValueError("serve_plan together with curriculum: a plan and a curriculum write the same serve override buffer")
        self.task, self.env = task, task.env
        env = self.env
        self.device = dev = torch.device(env.device)
        self.rows = env.num_rows                  # actor rows: num_envs x num_agents (T4: 2 actors per env)
        cfg.check(self.rows)
        self.base_num_obs, self.num_actions = env.obs_buf.shape[1], int(task.num_actions)
        self._history = history_mod.parse(history, self.base_num_obs, self.num_actions)      # the width of the network's rows: resolved, with every refusal, first
        self.num_obs = self.base_num_obs if self._history is None else self._history["width"]
        self.seed = int(seed)
        dist = torch.distributed
        initialised = dist.is_available() and dist.is_initialized()
        if force and not initialised:
            raise RuntimeError("PPOTrainer(force=True) needs an initialised torch.distributed process group")
        self.group = group
        self.multi = initialised and (dist.get_world_size(group) > 1 or bool(force))
        self.world = dist.get_world_size(group) if self.multi else 1
        self.rank = dist.get_rank(group) if self.multi else 0
        H, n, mb = cfg.horizon_length, self.rows, cfg.minibatch_size
        self.curriculum = None
        serve_seed = scene.stream_seed(self.seed, scene.STREAM_SERVES)
        if serve_plan is not None:
            task._serve_plan = env.set_serve_plan(serve_plan, paired=serve_paired, seed=serve_seed)
        elif curriculum is not None:
            self.curriculum = env.set_serve_curriculum(**dict(curriculum), seed=serve_seed, horizon=H)
        self.adr = self.randomization = None
        tables_seed = scene.stream_seed(self.seed, scene.STREAM_TABLES)
        if randomization is not None and randomization is not False:
            if randomization is True:
                randomization = scene.reset_randomization_plan(task.randomization_params, dof_rows=task.DR_DOF_ROWS, mass_rows=task.DR_MASS_ROWS)
                if not randomization["tables"]:
                    raise ValueError("randomization=True: the task cfg's randomization_params name no actor parameter of the humanoid")
            self.randomization = randomization
            rr = env.set_reset_randomization(randomization, seed=tables_seed)
            rr.apply(torch.zeros(rr.reset_rows * env.num_envs, dtype=torch.int64, device=dev))   # the first application draws every env's columns: training starts randomised
        elif adr is not None:
            self.adr = adr_mod.AutoRandomizer(env, **dict(adr), seed=tables_seed, horizon=H)
        randomizer = self.adr if self.adr is not None else (env.reset_randomization if self.randomization is not None else None)
        # privileged critic inputs: their width sizes the critic's first layer, so it is resolved — with every refusal — before the network is built
        self._critic_inputs = None
        if critic_inputs:
            tabs = env.dr_tables
            self._critic_inputs = critic_input_mod.columns(critic_inputs, env.DR_TABLE_ROWS, None if tabs is None else
                                                           [k for k, t in zip(env.DR_TABLE_ROWS, tabs) if t is not None],
                                                           delay_range("action_delay", action_delay), delay_range("obs_delay", obs_delay), self.base_num_obs)
        P = self._critic_inputs["P"] if self._critic_inputs else 0
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            actor, critic = self._mlp(self.num_actions), self._mlp(1, self.num_obs + P)
        # the log-std gradient in the slots right after the heads' gradients: one collective carries both
        self.net = NativeActorCritic(actor, critic, self.num_obs, dev, normalize_input=cfg.normalize_input, head_grad_extra=self.num_actions, num_priv=P)
        self.learner = self.net.learner
        with torch.no_grad():
            self.net.sigma.fill_(cfg.sigma_init)
        self.logstd = self.net.sigma.data                                   # a2c_network.sigma of the checkpoint
        self.value_rms = RunningMeanStd(1, dev) if cfg.normalize_value else None
        self.roll_net = self.learner.net.sibling()                          # the rollout's activation buffers apart from the minibatch's
        self.col = RolloutCollector(env, self.roll_net, horizon=H, gamma=cfg.gamma, tau=cfg.tau, reward_scale=cfg.reward_scale,
                                    sigma=torch.exp(self.logstd), seed=sampler_stream_seed(self.seed),   # ranks under seed + r share no exploration noise, and none is the env's noise
                                    action_delay=action_delay, obs_delay=obs_delay, latency_seed=scene.stream_seed(self.seed, scene.STREAM_LATENCY),
                                    env_id_offset=task._env_id_offset, serve=self.curriculum if self.curriculum is not None else task._serve_plan,
                                    randomizer=randomizer, critic_input=critic_inputs or None, history=self._history, obs_noise=obs_noise, obs_drop=obs_drop,
                                    action_noise=action_noise, action_drop=action_drop, sensor_columns=sensor_columns,
                                    sensor_seed=scene.stream_seed(self.seed, scene.STREAM_SENSOR), task=task)
        if self._critic_inputs is not None:
            assert self.col.critic_input.record() == self._critic_inputs
        self.g_logstd = self.learner.grad_extra
        self.loss = LossGrad(self.num_actions, mb, dev, cfg, d_logstd=self.g_logstd)
        self.opt = DeviceAdam(self.learner.parameters() + [self.logstd], self.learner.gradients() + [self.g_logstd], cfg.learning_rate,
                              max_norm=cfg.grad_norm, truncate=cfg.truncate_grads, init_scale=cfg.init_scale if cfg.mixed_precision else 1.0,
                              growth_interval=cfg.growth_interval, dynamic=cfg.mixed_precision, world=self.world)
        # the gradient all-reduce: sums left in place, averaged inside the Adam kernel
        self.buckets = D.GradientBuckets(group, force=force, mean=False) if self.multi else None
        total = H * n
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.old_nlp, self.adv, self.old_v, self.ret = z(total), z(total), z(total), z(total)
        self.steps_per_epoch = cfg.mini_epochs * (total // mb)
        self.stats = z(self.steps_per_epoch, 8)
        self.ep_ret, self.ep_len = z(n), z(n)                              # the running episode of every row (unscaled rewards)
        self.meter = GameMeter(env.num_envs, n // env.num_envs, cfg.games_to_track, dev)     # rl_games' score: per rank, as in rl_games
        self.last_mean_rewards = NO_SCORE                                  # the score of the best checkpoint so far (fit)
        self.epoch, self.frame = 0, 0
        self.loaded_latency = None                                         # load(): the "latency" of the checkpoint resumed from
        self.loaded_sensor = None                                          # load(): its "sensor", likewise
        self.outcome = task.enable_outcomes() if outcomes else None         # pp_ta_outcome, int64 [16] (include/ppenv_ta_outcome.h)
        if self.multi:
            self._broadcast_start()

    @torch.no_grad()
    def _broadcast_start(self):
        """Rank 0's fp32 parameters, log-std and input / value statistics (running and the fp32 images the kernels read) to every rank."""
        dist = torch.distributed
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        tensors = self.learner.masters() + [self.logstd]                    # (parameters(), with an asymmetric critic's layer 1 as its one contiguous tensor)
        for rms in (self.learner.rms, self.value_rms, self.learner.priv_rms):
            if rms is not None:
                tensors += [rms.running_mean, rms.running_var, rms.count, rms.mean, rms.inv_std]
        for t in tensors:
            dist.broadcast(t, src, group=self.group)
        self.learner.sync_weights()
        self.col.sigma.copy_(torch.exp(self.logstd))

    def _mlp(self, n_out, num_in=None):
        d, out = self.num_obs if num_in is None else num_in, []
        for u in list(self.cfg.units) + [n_out]:
            lin = torch.nn.Linear(d, u)
            out.append((lin.weight.detach(), lin.bias.detach()))
            d = u
        return out

    def set_capture(self, capture):
        """Record videos while training: `capture` (render.TrainingCapture over a Renderer of THIS task; None: stop) gets one on_step() after
        every control step of the rollout.  Its step count starts at epoch x horizon_length, so a resumed run continues the numbering of
        the files.  Rendering reads the env's state and writes its own tensors: the run is bitwise the run without it.  Data-parallel:
        rank 0 alone captures; the other ranks ignore the call."""
        if capture is not None and capture.renderer.task is not self.task:
            raise ValueError("the recorder renders another task")
        if capture is None or self.rank != 0:
            self.col.on_step = None
            return
        capture.start_step = self.epoch * self.cfg.horizon_length
        self.col.on_step = capture.on_step

    def serve(self):
        """The serve plan's resolved cells and pairing, or None without a plan."""
        plan = self.task._serve_plan
        return None if plan is None else dict(cells=[{k: [float(v[0]), float(v[1])] for k, v in c.items()} for c in plan.cells], paired=plan.paired)

    def clear_serve(self):
        """The built-in serves again: the plan or the curriculum is dropped and the collector launches nothing for it any more."""
        self.col.serve = None
        self.task.clear_serve_plan()
        self.env.clear_serve_curriculum()
        self.curriculum = None

    def clear_randomization(self):
        """No randomisation again: the plan or the ADR state is dropped, the env's tables are cleared and the collector launches nothing for
        them any more."""
        self.col.randomizer = None
        if self.adr is not None or self.randomization is not None:
            self.env.clear_randomization()
        self.adr = self.randomization = None

    def critic_inputs(self):
        """The record of the privileged critic inputs — dict(names=[...], columns=[one count per name], P=the sum) — or None without any."""
        r = self._critic_inputs
        return None if r is None else dict(names=list(r["names"]), columns=[int(c) for c in r["columns"]], P=int(r["P"]))

    def history(self):
        """The record of the observation and action history — dict(obs=Ho, actions=Ha, num_obs=n, num_actions=A, width=W) — or None without one."""
        return None if self._history is None else dict(self._history)

    def latency(self):
        """The control dt in seconds and the two delay ranges [lo, hi] in control steps ([0, 0]: that path is not delayed)."""
        return dict(control_dt=self.env.control_dt, action_delay=list(self.col.action_delay), obs_delay=list(self.col.obs_delay))

    def sensor(self):
        """The four level ranges [lo, hi] ([0, 0] twice: that path has no sensor line) and the four column specs as given, or None with
        no sensor line at all."""
        if self.col.obs_sensor is None and self.col.act_sensor is None:
            return None
        return dict(**{axis: list(r) for axis, r in self.col.sensor_levels.items()}, columns=dict(self.col.sensor_columns))

    # -- the steps of an epoch --
    def collect(self):
        """One horizon; with normalize_value the value column is de-normalised and GAE re-run on it (the collector's own GAE ran on the
        network's normalised output)."""
        col = self.col
        col.collect()
        if self.value_rms is not None:
            _denorm_(col.values, self.value_rms)
            gae(col.rewards, col.values, col.dones, self.cfg.gamma, self.cfg.tau, self.cfg.reward_scale, col.advantages, col.returns)
        return col

    @torch.no_grad()
    def prepare(self):
        """old_neglogp on the stored actions, the value statistics (rl_games: updated with the values, then with the returns, each normalised
        right after its update), advantages = returns - values normalised."""
        col, H, n, A = self.col, self.cfg.horizon_length, self.rows, self.num_actions
        total = H * n
        act, mu = col.actions.reshape(total, A), col.head[:H].reshape(total, A + 1)[:, :A]
        sg = col.sigma
        self.old_nlp.copy_((((act - mu) / sg) ** 2).sum(1).mul_(0.5).add_(HALF_LOG_2PI * A).add_(torch.log(sg).sum()))
        values, returns = col.values[:H].reshape(total, 1), col.returns.reshape(total, 1)
        adv = col.advantages.reshape(total)
        if self.cfg.normalize_advantage:
            self.adv.copy_((adv - adv.mean()) / (adv.std() + 1e-8))
        else:
            self.adv.copy_(adv)
        if self.value_rms is not None:
            v = values.contiguous()
            self.value_rms.update(v)
            self.old_v.copy_(_norm(v, self.value_rms).view(-1))
            r = returns.contiguous()
            self.value_rms.update(r)
            self.ret.copy_(_norm(r, self.value_rms).view(-1))
        else:
            self.old_v.copy_(values.view(-1))
            self.ret.copy_(returns.view(-1))

    def minibatch_step(self, lo, stats_row):
        """One optimizer step on rows lo .. lo + minibatch_size of the prepared epoch."""
        cfg, col, A = self.cfg, self.col, self.num_actions
        mb, total = cfg.minibatch_size, cfg.horizon_length * self.rows
        sl = slice(lo, lo + mb)
        obs = col.obs[:cfg.horizon_length].reshape(total, self.num_obs)[sl]
        priv = None if col.priv is None else col.priv[:cfg.horizon_length].reshape(total, col.priv.shape[2])[sl]
        mu, value = self.learner.forward(obs, priv, update_stats=cfg.normalize_input)
        old_mu = col.head[:cfg.horizon_length].reshape(total, A + 1)[sl, :A]
        d_head = self.loss(mu, value, col.actions.reshape(total, A)[sl], old_mu, col.sigma, self.old_nlp[sl], self.adv[sl], self.old_v[sl],
                           self.ret[sl], self.logstd, self.opt.scale, stats_row)
        if self.buckets is not None:
            self.learner.backward(d_head, on_grads=self._on_grads)
            self.buckets.wait()                                              # the stream waits for the collectives, the host does not
        else:
            self.learner.backward(d_head)
        self.opt.step()
        self.learner.sync_weights()

    def _on_grads(self, name, tensors):
        """The backward's per-layer callback: the heads' bucket takes the log-std gradient (adjacent in memory) along: layers + 1 collectives."""
        self.buckets(name, list(tensors) + [self.g_logstd] if name == "heads" else tensors)

    def learn(self):
        total, mb = self.cfg.horizon_length * self.rows, self.cfg.minibatch_size
        k = 0
        for _ in range(self.cfg.mini_epochs):
            for lo in range(0, total, mb):
                self.minibatch_step(lo, self.stats[k])
                k += 1

    @torch.no_grad()
    def _episodes(self):
        """Sum of returns, sum of lengths and count of the episodes that finished in the horizon (vectorised over the horizon)."""
        col, H = self.col, self.cfg.horizon_length
        r, d = col.rewards, col.dones.bool()
        cs = r.cumsum(0)
        t = torch.arange(H, device=self.device).view(H, 1)
        last = torch.where(d, t, -1).cummax(0).values                          # last done at or before t
        prev = torch.cat([torch.full_like(last[:1], -1), last[:-1]])           # ... strictly before t
        fresh = prev < 0
        ret = cs - torch.where(fresh, 0.0, cs.gather(0, prev.clamp(min=0))) + torch.where(fresh, self.ep_ret, 0.0)
        length = (t - prev).float() + torch.where(fresh, self.ep_len, 0.0)
        df = d.float()
        out = torch.stack([(ret * df).sum(), (length * df).sum(), df.sum()])
        end = last[-1]
        self.ep_ret.copy_(torch.where(end < 0, self.ep_ret + cs[-1], cs[-1] - cs.gather(0, end.clamp(min=0).view(1, -1)).view(-1)))
        self.ep_len.copy_(torch.where(end < 0, self.ep_len + H, (H - 1 - end).float()))
        return out

    @torch.no_grad()
    def _outcomes(self):
        """outcome_windows (cumulative, this rank's), outcome_envs = last_envs and outcome_<name> = last[k] / last_envs as fp32 (0 before the
        first window), 0-dim device tensors.  Data-parallel: last[] and last_envs are summed over the ranks (one int64 all-reduce)."""
        o = _lib.TAOutcome
        t = self.outcome
        last = t[o.last_envs.offset // 8:o.last.offset // 8 + len(_lib.TA_OUTCOME_NAMES)].clone()        # last_envs, last[5]: adjacent words
        if self.multi:
            torch.distributed.all_reduce(last, op=torch.distributed.ReduceOp.SUM, group=self.group)
        rates = last[1:].float() / last[0].clamp(min=1).float()
        out = dict(outcome_windows=t[o.windows.offset // 8].clone(), outcome_envs=last[0])
        out.update({f"outcome_{name}": rates[k] for k, name in enumerate(_lib.TA_OUTCOME_NAMES)})
        return out

    def train_epoch(self):
        """One epoch; no host synchronisation.  -> dict of 0-dim device tensors: the STATS averaged over the epoch's minibatch steps, the
        loss scale, the steps skipped in this epoch, the last gradient norm, the mean return / length of the episodes finished in the
        horizon (unscaled rewards; 0 when none finished), and rl_games' score after this horizon: meter_return / meter_length, the running
        means of the last meter_games <= games_to_track finished games (agent 0's unscaled return; 0 games: nothing to judge yet).
        Data-parallel: every rank keeps its own meter, as in rl_games, and every rank returns RANK 0's — the rank that judges and writes
        the checkpoints — so that the returned statistics are the same on all ranks (one 40-byte broadcast per epoch)."""
        skipped0 = self.opt.fields()["skipped"].clone()
        self.net.train()
        self.collect()
        # the horizon into the curriculum, then into ADR (curriculum.HorizonStage.epoch): data-parallel, the ranks' totals are summed in that order
        reduce = (lambda tot: torch.distributed.all_reduce(tot, op=torch.distributed.ReduceOp.SUM, group=self.group)) if self.multi else None
        staged = [stage.epoch(reduce) for stage in (self.curriculum, self.adr) if stage is not None]
        self.meter.update(self.col.rewards, self.col.dones)
        score = self.meter.snapshot()
        ep = self._episodes()
        self.prepare()
        self.learn()
        self.col.sigma.copy_(torch.exp(self.logstd))
        self.col.next_horizon()
        self.net.eval()
        self.epoch += 1
        self.frame += self.cfg.horizon_length * self.rows * self.world
        mean = self.stats.mean(0)
        if self.multi:                                                       # one all-reduce: the rank means' sum, the episode sums
            g = torch.cat([mean[:len(STATS)], ep])
            torch.distributed.all_reduce(g, op=torch.distributed.ReduceOp.SUM, group=self.group)
            mean, ep = g[:len(STATS)] / self.world, g[len(STATS):]
            src = torch.distributed.get_global_rank(self.group, 0) if self.group is not None else 0
            torch.distributed.broadcast(score, src, group=self.group)
        f = self.opt.fields()
        out = {k: mean[i] for i, k in enumerate(STATS)}
        n = ep[2].clamp(min=1.0)
        out.update(scale=f["scale"], skipped=f["skipped"] - skipped0, grad_norm=f["grad_norm"], episodes=ep[2], mean_return=ep[0] / n,
                   mean_length=ep[1] / n)
        score = self.meter.fields(score)
        out.update(meter_return=score["mean_reward"], meter_length=score["mean_length"], meter_games=score["current_size"])
        if self.outcome is not None:
            out.update(self._outcomes())
        for named in staged:
            out.update(named)
        return out

    # -- checkpoints --
    def state_dict(self):
        model = self.net.to_rlgames_state_dict()
        if self.value_rms is not None:
            for k in ("running_mean", "running_var", "count"):
                model[f"value_mean_std.{k}"] = getattr(self.value_rms, k).detach().clone()
        # the fp32 statistics the kernels read, as the update kernel left them (RunningMeanStd.refresh derives them from the fp64 running
        # statistics in torch and can differ in the last bit): a resumed run normalises exactly as the uninterrupted one
        stats = {f"{name}.{k}": getattr(rms, k).detach().clone() for name, rms in (("running_mean_std", self.learner.rms), ("value_mean_std", self.value_rms),
                                                                                  ("critic_mean_std", self.learner.priv_rms))
                 if rms is not None for k in ("mean", "inv_std")}
        sd = {"model": model, "epoch": self.epoch, "frame": self.frame, "optimizer": self.opt.state_dict(), "normalizer": stats,
              "meter": self.meter.state_dict(), "last_mean_rewards": float(self.last_mean_rewards),
              "latency": {k: v for k, v in self.latency().items() if k != "control_dt"}}
        rz, state = self.randomization, lambda stage: None if stage is None else stage.state_dict()
        plan = None if rz is None else {"frequency": int(rz["frequency"]),
                                        "tables": {k: {f: (list(v) if isinstance(v, (tuple, list)) else v) for f, v in t.items()} for k, t in rz["tables"].items()}}
        for key, record in (("serve", self.serve()), ("curriculum", state(self.curriculum)), ("randomization", plan), ("adr", state(self.adr)),
                            ("critic_inputs", self.critic_inputs()), ("history", self.history()), ("sensor", self.sensor())):
            if record is not None:                                           # an absent feature leaves no key
                sd[key] = record
        return sd

    def save(self, path):
        """Data-parallel: rank 0 writes, the other ranks return (their parameters and optimizer state are rank 0's)."""
        if self.rank != 0:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.state_dict(), path)

    def load(self, path):
        """Resume from save(): network, input and value statistics, log-std, optimizer moments, step count and loss scale, epoch / frame.
        Data-parallel: every rank loads the same file (rank 0's), so all resume identical, each with rank 0's input and value statistics."""
        ck = torch.load(path, map_location=self.device, weights_only=True)
        critic_input_mod.check_record(ck.get("critic_inputs"), self._critic_inputs)   # first: other privileged columns raise before anything is overwritten
        history_mod.check_record(ck.get("history"), self._history)           # likewise: another history is another first layer
        for key, stage in (("curriculum", self.curriculum), ("adr", self.adr)):
            if stage is not None and key in ck:                              # likewise: other bins, then other dims, raise before anything else is overwritten.  A file without the key: the table starts fresh
                stage.load_state_dict(ck[key])
        sd, lr = ck["model"], self.learner
        actor, critic = layers_from_rlgames_state_dict(sd)
        with torch.no_grad():
            for i in range(len(lr.w32)):
                for j, layers in enumerate((actor, critic)):
                    lr.layer_weights(i)[j].copy_(layers[i][0])              # (layer 1 of an asymmetric critic: the actor's column view)
                    lr.b32[i][j].copy_(layers[i][1])
            lr.mu_w.copy_(actor[-1][0]); lr.mu_b.copy_(actor[-1][1])
            lr.value_w.copy_(critic[-1][0]); lr.value_b.copy_(critic[-1][1])
            self.logstd.copy_(sd["a2c_network.sigma"])
            for rms, prefix in ((lr.rms, "running_mean_std"), (self.value_rms, "value_mean_std"), (lr.priv_rms, "critic_mean_std")):
                if rms is not None:
                    for k in ("running_mean", "running_var", "count"):
                        getattr(rms, k).copy_(sd[f"{prefix}.{k}"])
                    rms.refresh()
                    for k in ("mean", "inv_std"):
                        if f"{prefix}.{k}" in ck.get("normalizer", {}):
                            getattr(rms, k).copy_(ck["normalizer"][f"{prefix}.{k}"])
            self.col.sigma.copy_(torch.exp(self.logstd))
        lr.sync_weights()
        self.opt.load_state_dict(ck["optimizer"])
        self.epoch, self.frame = int(ck["epoch"]), int(ck["frame"])
        if "meter" in ck:                                                    # checkpoints from before the score meter have neither
            self.meter.load_state_dict(ck["meter"])
        self.last_mean_rewards = float(ck.get("last_mean_rewards", NO_SCORE))
        self.loaded_latency = ck.get("latency")                              # what the file's run trained under; None: a file from before the key
        self.loaded_sensor = ck.get("sensor")                                # likewise; None: a run without a sensor line, or a file from before the key



# ---- the run loop -----------------------------------------------------------------------------------------------------------------
def fit(trainer, out_dir, name, print_every=10, max_epochs=None, capture=None, curriculum_every=0, curriculum_out=None, adr_every=0, adr_out=None):
    """rl_games' train loop around train_epoch(), restated from its published a2c_common.train (rl_games is absent offline: parity
    unpinned).  Runs until trainer.epoch reaches max_epochs (default cfg.max_epochs: the TOTAL, so a resumed trainer continues its
    numbering) or the score wins.  After every epoch, with ONE host read (here, not in train_epoch):
      - every cfg.save_frequency epochs and at the end: <out_dir>/nn/<name>.pth — the LATEST weights, as before;
      - when meter_games > 0, meter_return > trainer.last_mean_rewards and epoch >= cfg.save_best_after: last_mean_rewards = meter_return
        and <out_dir>/nn/<name>_best.pth is written (rl_games writes its best to <name>.pth and its latest to last_<name>...: here the
        existing file name keeps its meaning);
      - if that new best also exceeds cfg.score_to_win: <out_dir>/nn/<name>_ep_<epoch>_rew_<meter_return>.pth, and the loop stops.
    Data-parallel: train_epoch() returns rank 0's score on every rank, so all ranks take the same decisions and leave in the same epoch;
    rank 0 alone writes (trainer.save).  print_every: rank 0 prints a line every so many epochs and at the end (0: never).
    -> dict(epochs: run by this call, epoch: the trainer's, stopped, reason: "max_epochs" | "score_to_win", best_score: last_mean_rewards
    (NO_SCORE while there is no best), paths: dict(latest, best, won: None where not written by this call), written: every path in order).
    capture: a render.TrainingCapture (trainer.set_capture is called with it): polled after every epoch's host read, closed before
    returning; the result then has `videos`, the files it wrote.
    curriculum_every: with a serve curriculum, rank 0 prints its table every so many epochs and at the end (0: never) — a second host read in
    those epochs — and rewrites curriculum_out (a json path) with it.
    adr_every, adr_out: the same for ADR's range table (adr.table_json / table_lines)."""
    cfg = trainer.cfg
    if capture is not None:
        trainer.set_capture(capture)
    total = int(cfg.max_epochs if max_epochs is None else max_epochs)
    nn_dir = os.path.join(out_dir, "nn")
    paths = dict(latest=None, best=None, won=None)
    written, ran, stopped = [], 0, False
    frame0, t0 = trainer.frame, time.perf_counter()

    def save(kind, path):
        trainer.save(path)                                                   # rank 0 only
        paths[kind] = path
        written.append(path)

    def table(module, stage, every, path, epoch, last):
        """Rank 0, every `every` epochs and at the end: the table of the trainer's `stage` ("curriculum" / "adr"; the module's table_json /
        table_lines) printed and `path` rewritten."""
        if every and getattr(trainer, stage) is not None and (epoch % every == 0 or last) and trainer.rank == 0:
            rows = module.table_json(getattr(trainer, stage), epoch)
            print("\n".join(module.table_lines(rows)), flush=True)
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as fh:
                    json.dump(rows, fh, indent=1)

    while trainer.epoch < total and not stopped:
        res = trainer.train_epoch()
        ran += 1
        epoch = trainer.epoch
        keys = [k for k in res if res[k].dim() == 0]                        # the curriculum's [B] tensors are read when its table is printed
        vals = dict(zip(keys, torch.stack([res[k].detach().double() for k in keys]).tolist()))     # the epoch's only host read
        if capture is not None:
            capture.poll()
        score, games = vals["meter_return"], int(vals["meter_games"])
        if games > 0 and score > trainer.last_mean_rewards and epoch >= cfg.save_best_after:
            trainer.last_mean_rewards = score
            save("best", os.path.join(nn_dir, f"{name}_best.pth"))
            if score > cfg.score_to_win:
                save("won", os.path.join(nn_dir, f"{name}_ep_{epoch}_rew_{score}.pth"))
                stopped = True
        last = stopped or epoch >= total
        if epoch % cfg.save_frequency == 0 or last:
            save("latest", os.path.join(nn_dir, f"{name}.pth"))
        if print_every and (epoch % print_every == 0 or last) and trainer.rank == 0:
            dt = time.perf_counter() - t0
            print(f"epoch {epoch} frames {trainer.frame} fps {(trainer.frame - frame0) / dt:.0f} loss {vals['loss']:.4g} a {vals['a_loss']:.4g} "
                  f"c {vals['c_loss']:.4g} kl {vals['kl']:.3g} clip {vals['clip_frac']:.3f} scale {vals['scale']:.0f} skipped {vals['skipped']:.0f} "
                  f"return {vals['mean_return']:.4g} length {vals['mean_length']:.1f} score {score:.6g} ({games} games)" +
                  ("".join(f" {name} {vals['outcome_' + name]:.3f}" for name in _lib.TA_OUTCOME_NAMES) +
                   f" ({vals['outcome_windows']:.0f} windows)" if "outcome_windows" in vals else ""), flush=True)
            if stopped:
                print(f"score {score} above score_to_win {cfg.score_to_win}: stopping", flush=True)
        table(curriculum_mod, "curriculum", curriculum_every, curriculum_out, epoch, last)
        table(adr_mod, "adr", adr_every, adr_out, epoch, last)
    out = dict(epochs=ran, epoch=trainer.epoch, stopped=stopped, reason="score_to_win" if stopped else "max_epochs",
               best_score=trainer.last_mean_rewards, paths=paths, written=written)
    if capture is not None:
        out["videos"] = capture.close()
        trainer.set_capture(None)
    return out


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def init_rank(backend="nccl", force=False):
    """The process group of a data-parallel run under torch.distributed.run (train.py's rank semantics): -> (rank, device).  nccl: one GPU per
    rank, cuda:LOCAL_RANK, the communicator bound to it (device_id, as bench.py); gloo: ranks may share cuda:LOCAL_RANK % device_count.
    force: a one-rank world (no launcher) is accepted and gets the group too."""
    rank, local_rank, world = D.rank_info()
    if world <= 1 and not force:
        raise SystemExit("--multi-gpu needs a world above 1: launch it with `python -m torch.distributed.run --nproc_per_node=N -m isaacgym_amd.ppo "
                         "--multi-gpu ...`, or pass --force-dist to run the collectives with one rank")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:              # a one-rank world without a launcher (--force-dist): any free port of this host
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
    dist = torch.distributed
    if backend == "nccl":
        dev = torch.device("cuda", local_rank)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dev = torch.device("cuda", local_rank % torch.cuda.device_count())
        torch.cuda.set_device(dev)
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, dev


def serve_cell_parse(flags):
    """--serve AXIS=V / AXIS=LO:HI flags -> [one cell dict] for PPOTrainer(serve_plan=), or None without flags.  The values stay text:
    serve.value_range and serve.resolve_cells judge them, with their own error texts, when the plan is set."""
    if not flags:
        return None
    cell = {}
    for flag in flags:
        axis, sep, v = str(flag).partition("=")
        if not sep:
            raise ValueError(f"--serve {flag!r}: expected AXIS=V or AXIS=LO:HI")
        parts = v.split(":")
        cell[axis.strip()] = parts[0] if len(parts) == 1 else tuple(parts)
    return [cell]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m isaacgym_amd.ppo", description="PPO (rl_games a2c_continuous) on the native env and network")
    ap.add_argument("--task", default="HumanoidPingpongTiltNESSparse27DOFG1")
    ap.add_argument("--num-envs", type=int, default=4096, help="envs per rank with --multi-gpu")
    ap.add_argument("--max-epochs", type=int, default=None, help="the total: a run resumed with --checkpoint continues its epoch numbering up to it")
    ap.add_argument("--checkpoint", default=None, help="resume from this nn/<task>.pth (every rank loads it)")
    ap.add_argument("--save-best-after", type=int, default=None, help="no nn/<task>_best.pth before this epoch (yaml: 3000)")
    ap.add_argument("--score-to-win", type=float, default=None, help="stop once the score exceeds it (yaml: 20000)")
    ap.add_argument("--games-to-track", type=int, default=None, help="finished games the score is the running mean of (rl_games: 100)")
    ap.add_argument("--minibatch-size", type=int, default=None, help="rows per rank with --multi-gpu")
    ap.add_argument("--cfg-dir", default=None, help="a reference cfg/ directory to compose the task and train yamls from")
    ap.add_argument("--out", default=None, help="run directory (default runs/<task>)")
    ap.add_argument("--seed", type=int, default=42, help="with --multi-gpu, rank r uses seed + r (train.py)")
    ap.add_argument("--print-every", type=int, default=10)
    ap.add_argument("--multi-gpu", action="store_true", help="data-parallel, one rank per process under python -m torch.distributed.run")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="nccl (RCCL) one GPU per rank; gloo: ranks may share a GPU")
    ap.add_argument("--force-dist", action="store_true", help="with --multi-gpu: accept a one-rank world and run the collectives anyway")
    ap.add_argument("--outcomes", action="store_true", help="27-dof task: report the reference's five outcome counts (TA:1164-1168) as rates of the envs per epoch")
    ap.add_argument("--action-delay", default="0", metavar="K|LO:HI", help="train under control latency of the command path: the env consumes the action of K "
                    "control steps ago (0..15), or of LO..HI steps ago, drawn per env at every episode start")
    ap.add_argument("--obs-delay", default="0", metavar="K|LO:HI", help="... of the sensing path: the policy sees the observation of K (or LO..HI) control steps ago")
    for path, what in (("obs", "the observations the policy sees"), ("action", "the commands the env consumes")):
        ap.add_argument(f"--{path}-noise", default="0", metavar="S|LO:HI", help=f"train under Gaussian noise of amplitude S x the column's scale on {what}, or of an "
                        "amplitude in LO..HI drawn per env at every episode start")
        ap.add_argument(f"--{path}-drop", default="0", metavar="P|LO:HI", help=f"... under sample dropouts: each control step, with probability P (0..1, or drawn in "
                        f"LO..HI per episode), {what} are the last delivered ones again in the hold columns")
        ap.add_argument(f"--{path}-noise-columns", default=None, metavar="SPEC", help="the noised columns and their scales: comma-separated NAME[=SCALE] or "
                        "LO:HI[=SCALE], e.g. ball_pos=1,ball_vel=4,60:67=0.5; default all=1")
        ap.add_argument(f"--{path}-drop-columns", default=None, metavar="SPEC", help="the columns a dropout holds: comma-separated NAME or LO:HI; default all")
    ap.add_argument("--serve", action="append", default=[], metavar="AXIS=V|AXIS=LO:HI", help="train on a serve plan: pin a serve axis (serve_speed, serve_tilt, "
                    "serve_tilt_z; the 27-dof task also ball_y, ball_z) or give its range; repeatable, all flags together are one cell over all envs")
    ap.add_argument("--curriculum", action="append", default=[], metavar="AXIS=LO:HI:BINS", help="an adaptive serve curriculum: cut the axis into BINS equal "
                    "bins; repeatable, the product of the axes are the bins (at most 256)")
    ap.add_argument("--curriculum-power", type=int, default=1, help="a bin's weight is (1 / its rank by mean return) to this power, 0 .. 4 (0: uniform bins)")
    ap.add_argument("--curriculum-mix", type=float, default=0.25, help="the share of the draws spread evenly over the bins, 0 .. 1")
    ap.add_argument("--curriculum-alpha", type=float, default=0.3, help="the weight of an epoch's mean return in a bin's running mean, (0, 1]")
    ap.add_argument("--curriculum-every", type=int, default=0, help="print the curriculum's table every so many epochs (0: never)")
    ap.add_argument("--curriculum-out", default=None, help="a json file rewritten with the table at each print")
    ap.add_argument("--randomize", action="store_true", help="train under reset-time domain randomisation: the actor parameters of the task cfg's "
                    "randomization_params (needs --cfg-dir, or a task whose cfg carries them), redrawn for an env when it resets")
    ap.add_argument("--adr", action="append", default=[], metavar="TABLE=START_LO:START_HI:LIMIT_LO:LIMIT_HI:STEP", help="automatic domain randomisation of "
                    "one table (dof_stiffness_scale, dof_damping_scale, link_mass_scale, restitution_scale, friction_scale): its range starts at "
                    "START and widens towards LIMIT by STEP per move; repeatable")
    ap.add_argument("--adr-boundary-frac", type=float, default=0.25, help="the share of the envs that play a game pinned to a boundary, 0 .. 1 (0: fixed ranges)")
    ap.add_argument("--adr-min-games", type=int, default=256, help="games a boundary gathers before it is judged")
    ap.add_argument("--adr-low", type=float, default=None, help="a boundary whose games' mean return is at or below this moves back in "
                    "(write a negative value in exponent form as --adr-low=-1e3)")
    ap.add_argument("--adr-high", type=float, default=None, help="a boundary whose games' mean return is at or above this moves outward")
    ap.add_argument("--adr-every", type=int, default=0, help="print ADR's range table every so many epochs (0: never)")
    ap.add_argument("--adr-out", default=None, help="a json file rewritten with the table at each print")
    ap.add_argument("--critic-inputs", default="", metavar="NAME[,NAME...]", help="privileged critic inputs (an asymmetric actor-critic): tables (needs "
                    "--randomize or --adr), latency (needs --action-delay or --obs-delay), raw_obs (needs --obs-delay); the critic alone sees them")
    ap.add_argument("--obs-history", type=int, default=0, metavar="Ho", help="the policy also sees the Ho observations it saw before (0..8): a frame stack "
                    "built on the device, for training under --obs-delay / --action-delay / --randomize / --adr")
    ap.add_argument("--action-history", type=int, default=0, metavar="Ha", help="... and its own last Ha clamped actions (0..8)")
    ap.add_argument("--capture-video", action="store_true", default=None, help="record videos of the training envs to <out>/videos (train.py: capture_video)")
    ap.add_argument("--capture-video-freq", type=int, default=None, help="control steps between the starts of two recordings (1464)")
    ap.add_argument("--capture-video-len", type=int, default=None, help="control steps one recording covers (100)")
    ap.add_argument("--capture-envs", default="0", help="comma-separated env ids to draw, side by side (at most 16)")
    ap.add_argument("--capture-size", default="320x240", help="WIDTHxHEIGHT of one env's picture")
    ap.add_argument("--capture-every", type=int, default=1, help="control steps between two frames of a recording")
    ap.add_argument("--capture-fps", type=float, default=30.0)
    ap.add_argument("--capture-samples", type=int, default=2, choices=(1, 2, 4), help="rays per pixel and axis: 2 is 2 x 2 supersampling")
    ap.add_argument("--capture-deferred", action="store_true", help="a drawn step records the posed primitives only; a recording's rays are cast in one batched "
                    "launch when it ends (render.Trajectory): the same files, byte for byte")
    ap.add_argument("--capture-trajectories", action="store_true", help="also write rl-video-step-<k>.traj.npz beside each video (records deferred): "
                    "python -m isaacgym_amd.render replay draws it again at any size, sample count and camera")
    ap.add_argument("--camera", choices=("side", "follow"), default="side", help="side: table and humanoid(s); follow: the reference viewer's follow-cam")
    args = ap.parse_args(argv)
    if args.force_dist and not args.multi_gpu:
        ap.error("--force-dist belongs to --multi-gpu")
    action_delay, obs_delay = delay_range("--action-delay", args.action_delay), delay_range("--obs-delay", args.obs_delay)
    flag = lambda key: "--" + key.replace("_", "-")
    sensors = {axis: (sensor_mod.drop_range if axis.endswith("_drop") else sensor_mod.sigma_range)(flag(axis), getattr(args, axis)) for axis in sensor_mod.AXES}
    sensor_columns = {f"{axis}_columns": getattr(args, f"{axis}_columns") for axis in sensor_mod.AXES}
    sensor_mod.check_specs(args.task, sensor_columns, flag)
    try:
        serve_plan, curriculum = serve_cell_parse(args.serve), None
        critic_inputs = critic_input_mod.parse(args.critic_inputs)
        history = history_mod.parse((args.obs_history, args.action_history))
        if args.curriculum:
            if serve_plan is not None:
                raise ValueError("--serve together with --curriculum: a plan and a curriculum write the same serve override buffer")
            curriculum_mod.check_parameters(args.curriculum_power, args.curriculum_mix, args.curriculum_alpha)
            curriculum = dict(bins=curriculum_mod.grid(curriculum_mod.grid_parse(args.curriculum)), power=args.curriculum_power, mix=args.curriculum_mix,
                              alpha=args.curriculum_alpha)
        adr = None
        if args.adr:
            if args.randomize:
                raise ValueError("--randomize together with --adr: a reset-time plan and ADR write the same randomisation tables")
            if args.adr_low is None or args.adr_high is None:
                raise ValueError("--adr needs --adr-low and --adr-high: the mean returns at which a boundary moves back in / outward")
            frac, games, low, high = adr_mod.check_parameters(args.adr_boundary_frac, args.adr_min_games, args.adr_low, args.adr_high)
            adr = dict(dims=adr_mod.check_dims(adr_mod.parse(args.adr)), boundary_frac=frac, min_games=games, t_low=low, t_high=high)
    except ValueError as e:
        ap.error(str(e))
    rank, seed, dev = 0, args.seed, None
    if args.multi_gpu:
        rank, dev = init_rank(args.dist_backend, force=args.force_dist)
        seed = args.seed + rank
    import isaacgym_amd
    over = {k: v for k, v in (("max_epochs", args.max_epochs), ("minibatch_size", args.minibatch_size), ("save_best_after", args.save_best_after),
                              ("score_to_win", args.score_to_win), ("games_to_track", args.games_to_track)) if v is not None}
    task_cfg = None
    if args.cfg_dir:
        composed = cfgyaml.compose(args.task, args.cfg_dir, overrides={"num_envs": args.num_envs})
        task_cfg = composed["task"]
        for key in ("capture_video", "capture_video_freq", "capture_video_len"):        # the composed cfg's keys are the defaults
            if getattr(args, key) is None and key in composed:
                setattr(args, key, composed[key])
        train = composed.get("train")        # the 27-dof task has no train yaml: the defaults (PPOConfig's, the Tilt yaml's)
        cfg = PPOConfig.from_train_cfg(train, task_cfg=task_cfg, **over) if train else PPOConfig(**over)
        cfg.check()
    else:
        cfg = PPOConfig(**over)
        cfg.check()
    if args.multi_gpu:
        task = isaacgym_amd.make(seed=seed, task=args.task, num_envs=args.num_envs, multi_gpu=True, device=dev, cfg=task_cfg)
    else:
        task = isaacgym_amd.make(seed=seed, task=args.task, num_envs=args.num_envs, cfg=task_cfg)
    tr = PPOTrainer(task, cfg, seed=seed, force=args.force_dist, outcomes=args.outcomes, action_delay=action_delay, obs_delay=obs_delay,
                    serve_plan=serve_plan, curriculum=curriculum, randomization=True if args.randomize else None, adr=adr, critic_inputs=critic_inputs,
                    history=history, sensor_columns=sensor_columns, **sensors)
    if rank == 0 and tr.sensor() is not None:
        print(sensor_mod.sensor_text(tr.sensor()), flush=True)
    if rank == 0 and tr.randomization is not None:
        print("reset-time randomisation: " + ", ".join(f"{k} {t['distribution']} {t['operation']} {t['range'][0]:g}..{t['range'][1]:g}"
                                                       for k, t in tr.randomization["tables"].items()), flush=True)
    if rank == 0 and adr is not None:
        print("\n".join(adr_mod.table_lines(adr_mod.table_json(tr.adr))), flush=True)
    if rank == 0 and serve_plan is not None:
        print("serve plan: " + ", ".join(f"{k} {v[0]:g}..{v[1]:g}" for k, v in tr.serve()["cells"][0].items()), flush=True)
    if rank == 0 and curriculum is not None:
        print(f"serve curriculum: {tr.curriculum.bins} bins, power {tr.curriculum.power}, mix {tr.curriculum.mix:g}, alpha {tr.curriculum.alpha:g}", flush=True)
    if rank == 0 and (action_delay[1] or obs_delay[1]):
        print(latency_text(tr.latency()), flush=True)
    if rank == 0 and tr.history() is not None:
        print(history_mod.text(tr.history()), flush=True)
    if rank == 0 and tr.critic_inputs() is not None:
        print(critic_input_mod.text(tr.critic_inputs(), tr.num_obs), flush=True)
    if args.checkpoint:
        tr.load(args.checkpoint)                                   # every rank: the same file
        if rank == 0:
            print(f"resumed {args.checkpoint} at epoch {tr.epoch}, best score {tr.last_mean_rewards}", flush=True)
    out = args.out or os.path.join("runs", args.task)
    capture = None
    if args.capture_video and rank == 0:
        from . import play, render
        renderer = play.make_renderer(task, args)
        capture = render.TrainingCapture(renderer, os.path.join(out, "videos"), freq=args.capture_video_freq or 1464, length=args.capture_video_len or 100,
                                         every=args.capture_every, fps=args.capture_fps, deferred=args.capture_deferred, trajectories=args.capture_trajectories)
    done = fit(tr, out, args.task, print_every=args.print_every, capture=capture, curriculum_every=args.curriculum_every, curriculum_out=args.curriculum_out,
               adr_every=args.adr_every, adr_out=args.adr_out)
    if rank == 0:
        for path in done.get("videos", []):
            print(f"saved {path} (video)", flush=True)
        for kind, path in done["paths"].items():
            if path is not None:
                print(f"saved {path} ({kind})" + (f" (ranks: {tr.world}, frames global)" if tr.multi else ""), flush=True)
    if args.multi_gpu:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return done


if __name__ == "__main__":
    main()
