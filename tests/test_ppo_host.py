"""PPOTrainer's host side (no GPU): the train-yaml mapping and its refusals, and the per-row loss gradient the loss kernel implements
(isaacgym_amd.ppo.loss_grad_reference, fp64) against torch autograd of the same loss."""
import json
import math
import os

import numpy as np
import pytest
import torch

from isaacgym_amd import ppo

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "task_cfgs.json")


def _train(name="HumanoidPingpongTiltG1"):
    with open(GOLDEN) as fh:
        return json.load(fh)[name]


def test_from_train_cfg_maps_the_tilt_yaml():
    d = _train()
    c = ppo.PPOConfig.from_train_cfg(d["train"], task_cfg=d["task"], minibatch_size=32768)
    assert (c.e_clip, c.critic_coef, c.learning_rate, c.grad_norm) == (0.2, 4.0, 2e-5, 10.0)
    assert (c.horizon_length, c.mini_epochs, c.minibatch_size) == (32, 5, 32768)
    assert c.normalize_value and c.normalize_input and c.normalize_advantage and c.mixed_precision and c.clip_value and c.truncate_grads
    assert c.sigma_init == -2.0 and c.fixed_sigma and c.reward_scale == 0.01 and c.gamma == 0.99 and c.tau == 0.95
    assert c.bounds_loss_coef == 1e-4 and c.entropy_coef == 0.0 and c.lr_schedule == "constant" and tuple(c.units) == tuple(ppo.UNITS)
    assert (c.max_epochs, c.save_frequency) == (200000, 1500)
    c.check(rows=4096)                               # 32 x 4096 rows: 4 minibatches


def test_from_train_cfg_refuses_what_it_does_not_run():
    d = _train()
    with pytest.raises(ValueError, match=r"minibatch_size: 4 .*8192.*32768"):
        ppo.PPOConfig.from_train_cfg(d["train"])     # yaml:74 `minibatch_size: 4 # 8192`
    with pytest.raises(ValueError, match=r"minibatch_size: 100"):
        ppo.PPOConfig.from_train_cfg(d["train"], minibatch_size=100)
    c = ppo.PPOConfig.from_train_cfg(d["train"], minibatch_size=8192)
    with pytest.raises(ValueError, match=r"minibatch_size: 8192 does not divide"):
        c.check(rows=100)
    with pytest.raises(ValueError, match=r"lr_schedule"):
        ppo.PPOConfig.from_train_cfg(d["train"], minibatch_size=8192, lr_schedule="adaptive")
    t = json.loads(json.dumps(d["train"]))
    t["params"]["network"]["space"]["continuous"]["fixed_sigma"] = False
    with pytest.raises(ValueError, match=r"fixed_sigma"):
        ppo.PPOConfig.from_train_cfg(t, minibatch_size=8192)
    task = json.loads(json.dumps(d["task"]))
    task["task"]["randomize"] = True
    with pytest.raises(ValueError, match=r"randomize"):
        ppo.PPOConfig.from_train_cfg(d["train"], task_cfg=task, minibatch_size=8192)


def test_every_golden_train_cfg_maps():
    with open(GOLDEN) as fh:
        cfgs = json.load(fh)
    for name, d in cfgs.items():
        if d["train"] is None:                       # the 27-dof task has no train yaml: PPOConfig's defaults
            continue
        c = ppo.PPOConfig.from_train_cfg(d["train"], task_cfg=d["task"], minibatch_size=8192)
        assert c.learning_rate == 2e-5 and c.horizon_length == 32


def _batch(rng, m, a, e_clip=0.2):
    """Random rows that cover both clip sides of the surrogate, ratios inside the range, active and inactive value clipping, mu beyond +-1.1."""
    logstd = rng.uniform(-2.2, -1.5, a)
    sg = np.exp(logstd)
    mu = rng.uniform(-1.6, 1.6, (m, a))
    actions = np.clip(mu + sg * rng.standard_normal((m, a)), -1, 1)
    z = (actions - mu) / sg
    nlp = 0.5 * (z * z).sum(1) + ppo.HALF_LOG_2PI * a + logstd.sum()
    log_ratio = rng.choice([-0.6, -0.05, 0.0, 0.05, 0.6], m) + rng.uniform(-0.02, 0.02, m)     # ratio far outside / inside the clip range
    old_nlp = nlp + log_ratio
    old_mu = mu + 0.1 * rng.standard_normal((m, a))
    old_sigma = sg * rng.uniform(0.9, 1.1, a)
    adv = rng.standard_normal(m)
    old_v = rng.standard_normal(m)
    value = old_v + rng.choice([-0.5, -0.1, 0.1, 0.5], m)        # |v - old_v| beyond and inside e_clip
    ret = rng.standard_normal(m)
    return dict(mu=mu, value=value, actions=actions, old_neglogp=old_nlp, old_mu=old_mu, old_sigma=old_sigma, advantages=adv, old_values=old_v,
                returns=ret, logstd=logstd)


def _autograd(b, e_clip, critic_coef, bounds_coef, entropy_coef, clip_value):
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in b.items()}
    mu, value, logstd = t["mu"].requires_grad_(), t["value"].requires_grad_(), t["logstd"].requires_grad_()
    a = mu.shape[1]
    nlp = 0.5 * (((t["actions"] - mu) / torch.exp(logstd)) ** 2).sum(1) + 0.5 * math.log(2 * math.pi) * a + logstd.sum()
    ratio = torch.exp(t["old_neglogp"] - nlp)
    adv = t["advantages"]
    a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - e_clip, 1 + e_clip))
    if clip_value:
        vc = t["old_values"] + (value - t["old_values"]).clamp(-e_clip, e_clip)
        c_loss = torch.max((value - t["returns"]) ** 2, (vc - t["returns"]) ** 2)
    else:
        c_loss = (t["returns"] - value) ** 2
    b_loss = ((mu - 1.1).clamp(min=0) ** 2 + (mu + 1.1).clamp(max=0) ** 2).sum(-1)
    entropy = torch.distributions.Normal(mu, torch.exp(logstd)).entropy().sum(-1)
    loss = a_loss.mean() + 0.5 * critic_coef * c_loss.mean() - entropy_coef * entropy.mean() + bounds_coef * b_loss.mean()
    loss.backward()
    return loss.item(), mu.grad.numpy(), value.grad.numpy(), logstd.grad.numpy(), ratio.detach().numpy()


@pytest.mark.parametrize("clip_value", [True, False])
@pytest.mark.parametrize("a", [1, 7, 27, 32])
def test_analytic_loss_gradient_matches_autograd(a, clip_value):
    rng = np.random.default_rng(a + 100 * clip_value)
    m, e_clip, cc, bc, ec = 512, 0.2, 4.0, 1e-4, 0.01
    b = _batch(rng, m, a, e_clip)
    loss, g_mu, g_v, g_ls, ratio = _autograd(b, e_clip, cc, bc, ec, clip_value)
    # the batch covers what it is meant to cover
    assert (ratio > 1 + e_clip).any() and (ratio < 1 - e_clip).any() and ((ratio > 1 - e_clip) & (ratio < 1 + e_clip)).any()
    assert (np.abs(b["mu"]) > 1.1).any()
    dv = np.abs(b["value"] - b["old_values"])
    assert (dv > e_clip).any() and (dv < e_clip).any()
    scale = 1024.0
    r = ppo.loss_grad_reference(**b, e_clip=e_clip, critic_coef=cc, bounds_loss_coef=bc, entropy_coef=ec, clip_value=clip_value, scale=scale)
    np.testing.assert_allclose(r["d_mu"] / scale, g_mu, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(r["d_value"] / scale, g_v, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(r["d_logstd"] / scale, g_ls, rtol=1e-10, atol=1e-14)
    assert math.isclose(r["loss"], loss, rel_tol=1e-12, abs_tol=1e-14)
    # the clipped value branch really is taken somewhere (its gradient is zero there)
    if clip_value:
        assert (r["d_value"] == 0).any()
