"""Privileged critic inputs on the MI355X (include/ppenv_critic_input.h; policy.NativeMLP(num_priv=)): the gather and the prepare launch
bit for bit against the numpy restatement (critic_input_reference) and against ppenv_mlp_prepare_input on the concatenated row; the actor
of a wide network is bitwise the narrow network's; the wide learner's gradients against fp32 autograd on an explicit two-tower model, with
the tolerances of test_policy_backward; and the actor's privileged columns stay exactly zero under the optimizer.  Need a real MI355X."""
import numpy as np
import pytest

import critic_input_reference as ref
from test_policy_mlp import _mlp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNITS = (256, 128)


# ------------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize("rows", [64, 130])
@pytest.mark.parametrize("num_agents", [1, 2])
def test_gather_is_the_numpy_restatement_bit_for_bit(rows, num_agents):
    """Sources of every kind at once — a 7-row table, a per-env scalar, an int32 [rows], a row-major [rows, 313] inside a wider buffer —
    for both num_agents; 130 rows: a ragged last tile and a ragged last wave.  `out` is a slice of a wider buffer whose other columns and
    rows must stay as they were."""
    import torch
    from isaacgym_amd import critic_input as ci
    gen = np.random.default_rng(rows + num_agents)
    n = rows // num_agents
    table = gen.standard_normal((7, n)).astype(np.float32)
    scalar = gen.standard_normal(n).astype(np.float32)
    scalar[0] = -0.0
    delays = gen.integers(0, 16, rows).astype(np.int32)
    delays[-1] = 2 ** 24 + 1                                                                   # rounds on conversion
    wide = gen.standard_normal((rows, 320)).astype(np.float32)
    host = [dict(array=table, table_major=True), dict(array=scalar, table_major=True), dict(array=delays, table_major=False),
            dict(array=wide[:, :313], table_major=False)]
    want = ref.gather(host, rows, num_agents)
    P = 7 + 1 + 1 + 313
    assert want.shape == (rows, P)
    dev = [torch.from_numpy(a).to(DEV) for a in (table, scalar, delays)] + [torch.from_numpy(wide).to(DEV)[:, :313]]      # the last: row stride 320
    labels = ("link_mass_scale", "friction_scale", "action_delay", "raw_obs")
    src = [ci.source("test", lab, t, h["table_major"]) for lab, t, h in zip(labels, dev, host)]
    assert [s.cols for s in src] == [7, 1, 1, 313] and src[3].stride == 320 and src[2].kind == 1
    g = ci.CriticInput.from_sources(src, rows, num_agents, DEV)
    assert g.P == P
    buf = torch.full((rows + 2, P + 5), 3.0, device=DEV)
    out = buf[1:-1, :P]
    g.gather(out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:-1, :P].view(np.uint32), want.view(np.uint32))
    assert (got[0] == 3.0).all() and (got[-1] == 3.0).all() and (got[:, P:] == 3.0).all()
    with pytest.raises(ValueError, match="CriticInput.gather: out must be float32"):
        g.gather(buf[1:-1, :P - 1])


# ------------------------------------------------------------------------------------------------------ 2. prepare
@pytest.mark.parametrize("num_obs, P", [(313, 1), (313, 7), (313, 8), (313, 71), (64, 64)])
def test_prepare_is_one_call_of_prepare_input_on_the_concatenated_row(num_obs, P):
    """prepare_input on the wide buffer, then prepare_critic_input: bitwise ppenv_mlp_prepare_input in ONE call on cat([obs, priv]) with
    concatenated statistics — and the numpy restatement.  (64, 64): an aligned col0; the others: an odd col0, and 313 + 8 / + 71 cross the
    64-column pad.  Rows with values beyond the clip and a row of negative zeros; 70 rows: a ragged last workgroup."""
    import torch
    from isaacgym_amd.policy import prepare_critic_input, prepare_input
    m = 70
    gen = torch.Generator().manual_seed(num_obs + P)
    k = num_obs + P
    kp = (k + 63) // 64 * 64
    x = torch.randn(m, k, generator=gen) * 3.0
    x[1] *= 100.0                                                                              # beyond the clip on both sides
    x[2] = -0.0
    mean, inv_std = torch.randn(k, generator=gen) * 0.5, torch.rand(k, generator=gen) + 0.5
    mean[num_obs:num_obs + 1] = 0.0                                                            # the negative zero survives where mean is 0
    xd, md, sd = x.to(DEV), mean.to(DEV), inv_std.to(DEV)
    want = torch.full((m, kp), float("nan"), dtype=torch.float16, device=DEV)
    prepare_input(want, xd, md, sd, 5.0)
    got = torch.full((m, kp), float("nan"), dtype=torch.float16, device=DEV)
    obs, priv = xd[:, :num_obs], xd[:, num_obs:]                                               # views: a row stride wider than either
    prepare_input(got, obs, md[:num_obs].contiguous(), sd[:num_obs].contiguous(), 5.0)
    before = got.clone()
    prepare_critic_input(got, priv, num_obs, md[num_obs:].contiguous(), sd[num_obs:].contiguous(), 5.0)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert bool((got[:, k:] == 0).all()) and torch.equal(got[:, :num_obs].view(torch.int16), before[:, :num_obs].view(torch.int16))
    assert bool((got[1, num_obs:k].abs() == 5.0).any()) and bool(torch.signbit(got[2, num_obs]))
    # the columns below col0 are not written at all: a poisoned buffer keeps them
    poison = torch.full((m, kp), 7.0, dtype=torch.float16, device=DEV)
    prepare_critic_input(poison, priv, num_obs, md[num_obs:].contiguous(), sd[num_obs:].contiguous(), 5.0)
    assert bool((poison[:, :num_obs] == 7.0).all()) and torch.equal(poison[:, num_obs:].view(torch.int16), want[:, num_obs:].view(torch.int16))
    host = np.full((m, kp), 7.0, np.float16)
    ref.prepare(host, x[:, num_obs:].numpy(), mean[num_obs:].numpy(), inv_std[num_obs:].numpy(), 5.0, num_obs)
    assert np.array_equal(poison.cpu().numpy().view(np.uint16), host.view(np.uint16))
    # without statistics: converted only
    prepare_critic_input(poison, priv, num_obs)
    ref.prepare(host, x[:, num_obs:].numpy(), None, None, 5.0, num_obs)
    assert np.array_equal(poison.cpu().numpy().view(np.uint16), host.view(np.uint16))


# ------------------------------------------------------------------------------------------------------ 3. the actor cannot see it
def test_actor_output_is_bitwise_the_narrow_networks_and_the_value_reads_the_columns():
    import torch
    from isaacgym_amd.policy import NativeMLP
    num_obs, P, num_act, m = 80, 71, 7, 130
    gen = torch.Generator().manual_seed(11)
    actor, critic_wide = _mlp(torch, num_obs, UNITS, num_act, gen), _mlp(torch, num_obs + P, UNITS, 1, gen)
    critic_narrow = [(critic_wide[0][0][:, :num_obs].contiguous(), critic_wide[0][1])] + critic_wide[1:]
    mean, var = torch.randn(num_obs, generator=gen), torch.rand(num_obs, generator=gen) + 0.5
    wide = NativeMLP(actor, critic_wide, num_obs, DEV, mean=mean, var=var, num_priv=P)
    narrow = NativeMLP(actor, critic_narrow, num_obs, DEV, mean=mean, var=var)
    assert wide.w[0].shape == (2, UNITS[0], 192) and narrow.w[0].shape == (2, UNITS[0], 128) and bool((wide.w[0][0][:, num_obs:] == 0).all())
    obs = (torch.randn(m, num_obs, generator=gen) * 2).to(DEV)
    priv = (torch.randn(m, P, generator=gen) * 2).to(DEV)
    mu_n, v_n = (t.clone() for t in narrow.forward(obs))
    mu_w, v_w = (t.clone() for t in wide.forward(obs, priv=priv))
    assert torch.equal(mu_w.view(torch.int32), mu_n.view(torch.int32))                          # added products with exact zeros add exactly
    priv2 = priv.clone()
    priv2[:, 40] += 1.0
    mu_2, v_2 = (t.clone() for t in wide.forward(obs, priv=priv2))
    assert torch.equal(mu_2.view(torch.int32), mu_n.view(torch.int32)) and not torch.equal(v_2, v_w)
    # priv=None: the privileged columns are zero — the value of the narrow critic (the same first-layer products, plus exact zeros)
    mu_0, v_0 = (t.clone() for t in wide.forward(obs))
    assert torch.equal(mu_0.view(torch.int32), mu_n.view(torch.int32)) and torch.equal(v_0.view(torch.int32), v_n.view(torch.int32))
    with pytest.raises(ValueError, match="no privileged columns"):
        narrow.forward(obs, priv=priv)
    with pytest.raises(ValueError, match="num_priv 71: the actor's first layer must be"):
        NativeMLP(critic_wide[:1] + actor[1:], critic_wide, num_obs, DEV, num_priv=P)


def test_torch_module_with_privileged_columns_backpropagates_and_round_trips_through_rl_games_keys():
    """NativeActorCritic(num_priv=): `net(obs, priv)` is differentiable, layer 1 is two parameters, and its rl_games state dict — a critic
    layer 1 wider than the actor's, `critic_mean_std.*` — builds the same network again."""
    import torch
    from isaacgym_amd.policy import NativeActorCritic
    num_obs, P, num_act, m = 80, 71, 7, 128
    gen = torch.Generator().manual_seed(5)
    actor, critic = _mlp(torch, num_obs, UNITS, num_act, gen), _mlp(torch, num_obs + P, UNITS, 1, gen)
    net = NativeActorCritic(actor, critic, num_obs, DEV, num_priv=P)
    obs, priv = (torch.randn(m, num_obs, generator=gen) * 2).to(DEV), (torch.randn(m, P, generator=gen) + 1).to(DEV)
    net.train()
    mu, value = net(obs, priv)
    (mu.square().mean() * 64.0 + value.square().mean() * 64.0).backward()
    shapes = [tuple(p.shape) for p in net.hidden_w]
    assert shapes == [(UNITS[0], num_obs), (UNITS[0], num_obs + P), (2, UNITS[1], UNITS[0])]
    assert all(p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.requires_grad)
    assert float(net.hidden_w[1].grad[:, num_obs:].abs().max()) > 0 and float(net.critic_mean_std.count) == m + 1
    sd = net.to_rlgames_state_dict()
    assert sd["a2c_network.actor_mlp.0.weight"].shape == (UNITS[0], num_obs) and sd["a2c_network.critic_mlp.0.weight"].shape == (UNITS[0], num_obs + P)
    assert sd["critic_mean_std.running_mean"].shape == (P,)
    again = NativeActorCritic.from_rlgames(sd, DEV)
    assert again.learner.num_priv == P
    net.eval(), again.eval()
    for rms in (net.learner.rms, net.learner.priv_rms):                                         # the fp32 images as a loaded network derives them (the update
        rms.refresh()                                                                          # kernel's own can differ in the last bit)
    with torch.no_grad():
        a, b = net(obs, priv), again(obs, priv)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------ 4. backward
@pytest.mark.parametrize("m", [64, 192])
def test_wide_backward_matches_fp32_autograd_and_the_actors_privileged_columns_stay_zero(m):
    """The comparison and the tolerances of test_policy_backward.test_native_backward_matches_fp32_autograd (rtol 1e-2 plus 1e-2 of each
    gradient's scale, mean error below 2e-3 of it), on a two-tower torch model whose critic takes [obs | priv].  Then three DeviceAdam steps."""
    import torch
    from isaacgym_amd.policy import NativeMLPLearner, RunningMeanStd
    from isaacgym_amd.ppo import DeviceAdam
    num_obs, P, num_act = 80, 71, 7
    gen = torch.Generator().manual_seed(m)
    actor, critic = _mlp(torch, num_obs, UNITS, num_act, gen), _mlp(torch, num_obs + P, UNITS, 1, gen)
    obs = torch.randn(m, num_obs, generator=gen) * 2.0 + 0.3
    priv = torch.randn(m, P, generator=gen) * 1.5 - 0.2
    learner = NativeMLPLearner(actor, critic, num_obs, DEV, num_priv=P)
    rms, prms = RunningMeanStd(num_obs, DEV), RunningMeanStd(P, DEV)
    learner.attach_running_mean_std(rms)
    learner.attach_priv_running_mean_std(prms)
    learner.forward(obs.to(DEV), priv.to(DEV), update_stats=True)
    assert float(prms.count) == m + 1
    d_head = torch.randn(m, num_act + 1, generator=gen)
    d_head[:, num_act] *= 3.0
    grads = [g.clone() for g in learner.backward(d_head.to(DEV))]
    torch.cuda.synchronize()
    x = torch.clamp((obs - rms.mean.cpu()) * rms.inv_std.cpu(), -5.0, 5.0)
    xp = torch.clamp((priv - prms.mean.cpu()) * prms.inv_std.cpu(), -5.0, 5.0)
    params = []

    def run(layers, h):
        for i, (w, b) in enumerate(layers):
            w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            params.append((w, b))
            h = h @ w.t() + b
            if i + 1 < len(layers):
                h = torch.nn.functional.elu(h)
        return h
    out = torch.cat([run(actor, x), run(critic, torch.cat([x, xp], 1))], dim=1)
    out.backward(d_head)
    nl = len(UNITS)
    a_p, c_p = params[:nl + 1], params[nl + 1:]
    want = ([a_p[0][0].grad, c_p[0][0].grad] + [torch.stack([a_p[i][0].grad, c_p[i][0].grad]) for i in range(1, nl)] +
            [torch.stack([a_p[i][1].grad, c_p[i][1].grad]) for i in range(nl)] + [a_p[nl][0].grad, a_p[nl][1].grad, c_p[nl][0].grad, c_p[nl][1].grad])
    names = ["w0_actor", "w0_critic"] + [f"w{i}" for i in range(1, nl)] + [f"b{i}" for i in range(nl)] + ["mu_w", "mu_b", "value_w", "value_b"]
    ps = learner.parameters()
    assert len(grads) == len(want) == len(ps) == len(names)
    assert ps[0].shape == (UNITS[0], num_obs) and ps[1].shape == (UNITS[0], num_obs + P)
    for name, g, w, p in zip(names, grads, want, ps):
        g = g.cpu()
        assert g.shape == w.shape == p.shape, (name, g.shape, w.shape, p.shape)
        scale = float(w.abs().max())
        err = (g - w).abs()
        print(f"{name}: max err {float(err.max()):.3g} mean err {float(err.mean()):.3g} scale {scale:.3g}")
        assert bool((err <= 1e-2 * w.abs() + 1e-2 * scale).all()), (name, float(err.max()), scale)
        assert float(err.mean()) < 2e-3 * scale, (name, float(err.mean()), scale)
    # three optimizer steps: the actor's privileged columns are no parameter, so they stay exactly zero in the master and in the fp16 image
    opt = DeviceAdam(ps, learner.gradients(), 1e-3, init_scale=1.0, dynamic=False)
    critic_before = learner.w32[0][1][:, num_obs:].clone()
    actor_before = learner.w32[0][0][:, :num_obs].clone()
    for _ in range(3):
        learner.forward(obs.to(DEV), priv.to(DEV))
        learner.backward(d_head.to(DEV))
        opt.step()
        learner.sync_weights()
    torch.cuda.synchronize()
    assert bool((learner.w32[0][0][:, num_obs:] == 0).all()) and bool((learner.net.w[0][0][:, num_obs:] == 0).all())
    assert float((learner.w32[0][1][:, num_obs:] != critic_before).float().mean()) > 0.99         # the critic's privileged weights have moved
    assert not torch.equal(learner.w32[0][0][:, :num_obs], actor_before)
    assert torch.equal(learner.net.w[0][1][:, :num_obs + P], learner.w32[0][1].half())
