"""PPOTrainer and its kernels (include/ppenv_ppo.h) on the MI355X: the loss gradient against fp64, the clip + Adam + loss scale against
torch, one trainer minibatch step against the PyTorch path, whole epochs on the tasks, determinism, checkpoints and a learning signal."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def _batch(rng, m, a):
    """Random rows covering both clip sides of the surrogate, ratios inside the clip range, active / inactive value clipping, |mu| > 1.1."""
    from isaacgym_amd import ppo
    logstd = rng.uniform(-2.2, -1.5, a)
    sg = np.exp(logstd)
    mu = rng.uniform(-1.6, 1.6, (m, a))
    actions = np.clip(mu + sg * rng.standard_normal((m, a)), -1, 1)
    z = (actions - mu) / sg
    nlp = 0.5 * (z * z).sum(1) + ppo.HALF_LOG_2PI * a + logstd.sum()
    old_nlp = nlp + rng.choice([-0.6, -0.05, 0.0, 0.05, 0.6], m) + rng.uniform(-0.02, 0.02, m)
    old_v = rng.standard_normal(m)
    b = dict(mu=mu, value=old_v + rng.choice([-0.5, -0.1, 0.1, 0.5], m), actions=actions, old_neglogp=old_nlp,
             old_mu=mu + 0.1 * rng.standard_normal((m, a)), old_sigma=sg * rng.uniform(0.9, 1.1, a), advantages=rng.standard_normal(m),
             old_values=old_v, returns=rng.standard_normal(m), logstd=logstd)
    return {k: v.astype(np.float32) for k, v in b.items()}


@pytest.mark.parametrize("a", [7, 27])
@pytest.mark.parametrize("m", [64, 8192, 32768])
def test_loss_kernel_matches_fp64(torch_cuda, m, a):
    torch = torch_cuda
    from isaacgym_amd import ppo
    rng = np.random.default_rng(m + a)
    b = _batch(rng, m, a)
    cfg = ppo.PPOConfig(entropy_coef=0.01)
    scale = 65536.0
    ref = ppo.loss_grad_reference(**b, e_clip=cfg.e_clip, critic_coef=cfg.critic_coef, bounds_loss_coef=cfg.bounds_loss_coef,
                                  entropy_coef=cfg.entropy_coef, clip_value=True, scale=scale)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    head = torch.zeros((m, a + 1), device="cuda")                   # mu | value as the heads write them: row stride a + 1
    head[:, :a], head[:, a] = d(b["mu"]), d(b["value"])
    old_head = torch.zeros((m, a + 1), device="cuda")
    old_head[:, :a] = d(b["old_mu"])
    lg = ppo.LossGrad(a, m, "cuda", cfg)
    sc = torch.full((1,), scale, device="cuda")
    args = (head[:, :a], head[:, a:], d(b["actions"]), old_head[:, :a], d(b["old_sigma"]), d(b["old_neglogp"]), d(b["advantages"]),
            d(b["old_values"]), d(b["returns"]), d(b["logstd"]), sc)
    outs = []
    for _ in range(2):
        stats = torch.zeros(8, device="cuda")
        dh = lg(*args, stats).clone()
        outs.append((dh, lg.d_logstd.clone(), stats))
    torch.cuda.synchronize()
    dh, dls, stats = (t.cpu().double().numpy() for t in outs[0])
    for got, want, what in ((dh[:, :a], ref["d_mu"], "d mu"), (dh[:, a], ref["d_value"], "d value"), (dls, ref["d_logstd"], "d logstd")):
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max(), err_msg=what)
    for i, k in enumerate(ppo.STATS):
        np.testing.assert_allclose(stats[i], ref[k], rtol=1e-5, atol=1e-6, err_msg=k)
    for x, y in zip(outs[0], outs[1]):                              # no atomics: bitwise reproducible
        assert torch.equal(x, y)


def _learner(torch, seed=0, a=27, num_obs=313):
    from isaacgym_amd.policy import UNITS, NativeMLPLearner
    g = torch.Generator().manual_seed(seed)

    def mlp(n_out):
        d, out = num_obs, []
        for u in UNITS + [n_out]:
            out.append(((torch.rand(u, d, generator=g) - 0.5) * 2 / math.sqrt(d), (torch.rand(u, generator=g) - 0.5) * 0.1))
            d = u
        return out
    return NativeMLPLearner(mlp(a), mlp(1), num_obs, "cuda")


@pytest.mark.parametrize("grad_std,clip_active", [(1e-2, True), (1e-5, False)])
def test_clip_adam_matches_torch(torch_cuda, grad_std, clip_active):
    """The real learner's parameter list (layer 1's K-padded gradient stride, the heads' slices of head_w / head_b) + a log-std."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    lr = _learner(torch)
    logstd = torch.full((27,), -2.0, device="cuda")
    g_logstd = torch.zeros(27, device="cuda")
    params, grads = lr.parameters() + [logstd], lr.gradients() + [g_logstd]
    scale, lrate = 1024.0, 1e-3
    opt = ppo.DeviceAdam(params, grads, lrate, max_norm=10.0, truncate=True, init_scale=scale, growth_interval=2000)
    # the torch path in fp64: its clip_grad_norm_ then sees the norm the kernels sum in fp64 (an fp32 norm of 14.4 M elements is itself off by
    # about 1e-6, which would move the clip coefficient, and exp_avg_sq with its square, by about as much)
    tp = [torch.nn.Parameter(p.detach().double().clone()) for p in params]
    topt = torch.optim.Adam(tp, lr=lrate, eps=1e-8, foreach=False)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for step in range(10):
        for gbuf in list(lr.grads["w"]) + list(lr.grads["b"]) + [lr.grads["head_w"], lr.grads["head_b"], g_logstd]:
            gbuf.copy_(torch.randn(gbuf.shape, device="cuda", generator=gen) * grad_std * scale)
        for p, g in zip(tp, grads):
            p.grad = g.detach().double() / scale
        norm = torch.nn.utils.clip_grad_norm_(tp, 10.0)
        assert (float(norm) > 10.0) == clip_active
        topt.step()
        opt.step()
        for i, (p, q) in enumerate(zip(params, tp)):
            q = q.detach()
            torch.testing.assert_close(p.double(), q, rtol=1e-6, atol=1e-7 * float(q.abs().max()), msg=f"step {step}: parameter {i}")
            st = topt.state[tp[i]]
            for mine, theirs, what in ((opt.exp_avg[i], st["exp_avg"], "exp_avg"), (opt.exp_avg_sq[i], st["exp_avg_sq"], "exp_avg_sq")):
                torch.testing.assert_close(mine.double(), theirs, rtol=1e-6, atol=1e-6 * float(theirs.abs().max()), msg=f"step {step}: {what} {i}")
    f = opt.fields()
    assert int(f["step"]) == 10 and int(f["skipped"]) == 0 and float(f["scale"]) == scale
    # the fp16 operand images after sync_weights are the casts of the same masters
    lr.sync_weights()
    net, u, na = lr.net, lr.net.units, lr.net.num_actions
    for i in range(len(u)):
        k = lr.w32[i].shape[-1]
        assert torch.equal(net.w[i][..., :k], lr.w32[i].half()), f"w {i}"
        assert torch.equal(net.b[i], lr.b32[i].half()), f"b {i}"
        if i:
            assert torch.equal(lr.wt[i], lr.w32[i].half().transpose(1, 2)), f"wt {i}"
    assert torch.equal(net.head_w[:na, :u[-1]], lr.mu_w.half()) and torch.equal(net.head_w[na:, u[-1]:], lr.value_w.half())
    assert torch.equal(net.head_b, torch.cat([lr.mu_b, lr.value_b]).half())


def test_nonfinite_gradient_skips_the_step(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import ppo
    p = [torch.randn(64, 40, device="cuda"), torch.randn(27, device="cuda")]
    g = [torch.randn(64, 48, device="cuda")[:, :40], torch.randn(27, device="cuda")]     # a strided gradient
    opt = ppo.DeviceAdam(p, g, 1e-3, init_scale=1024.0, growth_interval=3)
    read = lambda: {k: float(v) for k, v in opt.fields().items()}
    opt.step()
    s = read()
    assert (s["step"], s["skipped"], s["scale"]) == (1, 0, 1024.0)
    for bad in (float("inf"), float("nan")):
        before = [t.clone() for t in p + opt.exp_avg + opt.exp_avg_sq]
        scale0 = read()["scale"]
        g[0][3, 5] = bad                                   # an injected value in a gradient buffer
        opt.step()
        s = read()
        assert s["step"] == 1 and s["scale"] == scale0 * 0.5 and s["growth_tracker"] == 0
        for x, y in zip(before, p + opt.exp_avg + opt.exp_avg_sq):
            assert torch.equal(x, y)
        g[0][3, 5] = 0.5
    assert read()["skipped"] == 2
    scale0 = read()["scale"]
    for k in range(3):                                     # growth after growth_interval clean steps
        opt.step()
        s = read()
        assert s["scale"] == (scale0 * 2 if k == 2 else scale0)
    assert s["step"] == 4 and s["growth_tracker"] == 0


def _trainer(torch, task="HumanoidPingpongTiltNESSparse27DOFG1", num_envs=256, seed=3, **cfg):
    import isaacgym_amd
    from isaacgym_amd import ppo
    cfg.setdefault("minibatch_size", 8192)
    t = isaacgym_amd.make(seed=seed, task=task, num_envs=num_envs)
    return ppo.PPOTrainer(t, ppo.PPOConfig(**cfg), seed=seed)


def _params(tr):
    return [p.detach().clone() for p in tr.learner.parameters()] + [tr.logstd.clone()]


def test_minibatch_step_matches_pytorch_path(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.policy import NativeActorCritic
    tr = _trainer(torch)                                    # 256 envs x 32 = one 8192-row minibatch
    cfg, A = tr.cfg, tr.num_actions
    tr.collect()
    tr.prepare()
    lr = tr.learner
    actor = [(lr.w32[i][0].clone(), lr.b32[i][0].clone()) for i in range(len(lr.w32))] + [(lr.mu_w.clone(), lr.mu_b.clone())]
    critic = [(lr.w32[i][1].clone(), lr.b32[i][1].clone()) for i in range(len(lr.w32))] + [(lr.value_w.clone(), lr.value_b.clone())]
    ref = NativeActorCritic(actor, critic, tr.num_obs, "cuda:0")
    ref.running_mean_std.load_state_dict(lr.rms.state_dict())
    logstd = torch.nn.Parameter(tr.logstd.clone())
    params = list(ref._ordered()) + [logstd]
    opt = torch.optim.Adam(params, lr=cfg.learning_rate, eps=1e-8, foreach=False)
    total = cfg.horizon_length * tr.rows
    col = tr.col
    obs = col.obs[:cfg.horizon_length].reshape(total, tr.num_obs)
    act = col.actions.reshape(total, A)
    ref.train()
    mu, value = ref(obs)
    nlp = 0.5 * (((act - mu) / torch.exp(logstd)) ** 2).sum(1) + 0.5 * math.log(2 * math.pi) * A + logstd.sum()
    ratio = torch.exp(tr.old_nlp - nlp)
    adv, ov, ret = tr.adv, tr.old_v, tr.ret
    a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - cfg.e_clip, 1 + cfg.e_clip))
    v = value.view(-1)
    vc = ov + (v - ov).clamp(-cfg.e_clip, cfg.e_clip)
    c_loss = torch.max((v - ret) ** 2, (vc - ret) ** 2)
    b_loss = ((mu - 1.1).clamp(min=0) ** 2 + (mu + 1.1).clamp(max=0) ** 2).sum(-1)
    loss = a_loss.mean() + 0.5 * cfg.critic_coef * c_loss.mean() + cfg.bounds_loss_coef * b_loss.mean()
    scale = float(tr.opt.scale)
    (loss * scale).backward()
    for p in params:
        p.grad.div_(scale)
    want_grads = [p.grad.clone() for p in params]
    torch.nn.utils.clip_grad_norm_(params, cfg.grad_norm)
    opt.step()
    tr.minibatch_step(0, tr.stats[0])
    torch.cuda.synchronize()
    assert abs(float(tr.stats[0, 0]) - float(loss.detach())) <= 1e-4 * abs(float(loss.detach())) + 1e-6
    # the gradients (scaled in the trainer's buffers) against autograd's through the same backward kernels
    for i, (g, w) in enumerate(zip(lr.gradients() + [tr.g_logstd], want_grads)):
        err = float((g / scale - w).norm())
        assert err <= 1e-3 * float(w.norm()) + 1e-12, (i, err, float(w.norm()))
    # Adam's first step moves every element by about lr x sign(g): an element whose gradient is within rounding of 0 may step the other way in
    # one path (at most 2 lr apart); every other element agrees to the tolerance of the clip + Adam test.  The former are counted.
    flips = 0
    for p, q in zip(_params(tr), [t.detach() for t in params]):
        bad = ~torch.isclose(p, q, rtol=1e-6, atol=1e-7)
        flips += int(bad.sum())
        assert float((p - q).abs().max()) <= 2.01 * cfg.learning_rate
    n = sum(p.numel() for p in params)
    assert flips <= 1e-3 * n, f"{flips} of {n} elements differ"


def _epochs(torch, tr, k, sync_check=True):
    for e in range(k):
        if sync_check and e > 0 and hasattr(torch.cuda, "set_sync_debug_mode"):
            torch.cuda.set_sync_debug_mode("error")
            try:
                res = tr.train_epoch()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            res = tr.train_epoch()
    return res


@pytest.mark.parametrize("task,num_envs,epochs", [("HumanoidPingpongTiltG1", 4096, 3), ("HumanoidPingpongTiltNESSparse27DOFG1", 1024, 3),
                                                  ("Humanoid12PingpongTiltG1", 1024, 1)])
def test_train_epochs_end_to_end(torch_cuda, task, num_envs, epochs):
    torch = torch_cuda
    tr = _trainer(torch, task=task, num_envs=num_envs)
    if task == "Humanoid12PingpongTiltG1":
        assert tr.rows == 2 * num_envs                       # rl_games num_agents = 2
    res = _epochs(torch, tr, epochs)
    vals = {k: float(v) for k, v in res.items()}
    assert all(math.isfinite(v) for v in vals.values()), vals
    assert vals["scale"] > 0
    assert all(bool(torch.isfinite(p).all()) for p in _params(tr))
    assert tr.epoch == epochs and tr.frame == epochs * 32 * tr.rows


def test_same_seed_same_parameters(torch_cuda):
    torch = torch_cuda
    a, b = _trainer(torch, num_envs=512), _trainer(torch, num_envs=512)
    _epochs(torch, a, 2, sync_check=False)
    _epochs(torch, b, 2, sync_check=False)
    for x, y in zip(_params(a), _params(b)):
        assert torch.equal(x, y)


def test_checkpoint_serves_and_resumes(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd.policy import RLGamesPolicy
    a = _trainer(torch)
    a.train_epoch()
    path = str(tmp_path / "nn" / "run.pth")
    a.save(path)
    pol = RLGamesPolicy.load(path, "cuda:0")
    obs = a.env.obs_buf.clone()
    act, _ = pol.act(obs, deterministic=True)
    mu, _ = a.roll_net.forward(obs)
    assert torch.equal(act, mu.clamp(-1.0, 1.0))
    a.train_epoch()
    want = _params(a)
    b = _trainer(torch)
    b.train_epoch()
    with torch.no_grad():                                   # spoil everything load() must restore
        for p in b.learner.parameters():
            p.add_(0.5)
        b.logstd.add_(1.0)
        for m in b.opt.exp_avg + b.opt.exp_avg_sq:
            m.zero_()
        b.learner.rms.running_mean.add_(1.0)
        b.value_rms.running_var.mul_(3.0)
        b.opt.state.zero_()
    b.load(path)
    assert (b.epoch, b.frame) == (1, 32 * b.rows)
    b.train_epoch()
    for x, y in zip(want, _params(b)):
        assert torch.equal(x, y)


def test_learning_lowers_the_loss_on_a_fixed_batch(torch_cuda):
    torch = torch_cuda
    tr = _trainer(torch, learning_rate=1e-4)
    tr.collect()
    tr.prepare()
    total, A = 32 * tr.rows, tr.num_actions
    col = tr.col
    obs = col.obs[:32].reshape(total, tr.num_obs)
    stats = torch.zeros(8, device="cuda")

    def loss():
        mu, value = tr.learner.forward(obs, update_stats=False)
        tr.loss(mu, value, col.actions.reshape(total, A), col.head[:32].reshape(total, A + 1)[:, :A], col.sigma, tr.old_nlp, tr.adv, tr.old_v,
                tr.ret, tr.logstd, tr.opt.scale, stats)
        return float(stats[0])
    before = loss()
    tr.learn()                                               # 5 mini-epochs
    after = loss()
    assert math.isfinite(after) and after < before, (before, after)
