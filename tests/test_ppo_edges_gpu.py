"""The PPO trainer's kernels and bookkeeping on the MI355X at the shapes and switches the trainer's own tests do not reach, each against a
plain fp64 reference (tests/ppo_reference.py, ppo.loss_grad_reference, torch fp64 Adam): collect() + prepare() on real rollouts, the loss
kernel on ragged and tiny batches and every switch, DeviceAdam's vector / element paths, launch shapes and a 2100-step run, RunningMeanStd
at one column and half a million rows, GAE's edges.  Every test prints its worst error next to its bound.  Tolerances are the existing
tests' (test_ppo_gpu.py, test_policy_backward.py, test_collector.py), bounds derived from the fp64 reference, or — for the long run —
torch's own fp32 deviation from fp64; none was read off the code under test."""
import ctypes as C
import math

import numpy as np
import pytest

import ppo_reference as R
from ppo_reference import adv_bound, nlp_bound, norm_bound

pytestmark = pytest.mark.gpu

U32 = R.U32
PPENV_EINVAL = -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _report(what, err, bound):
    """Worst error over bound (element-wise), printed; -> that ratio."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratios = (err / np.where(bound > 0, bound, 1.0)).reshape(-1)
    at = int(ratios.argmax())
    print(f"  {what}: worst error / bound {ratios[at]:.3g} (error {err.reshape(-1)[at]:.3g}, bound {bound.reshape(-1)[at]:.3g}); "
          f"largest error {float(err.max()):.3g}")
    return float(ratios[at])


# ======================================================================================================================================
# 1. collect() + prepare() on real rollouts
# ======================================================================================================================================
def _rms_state(rms):
    return float(rms.running_mean.cpu()), float(rms.running_var.cpu()), float(rms.count.cpu())


def _denorm_bound(raw, state, eps=1e-5):
    """fp32 bound of clamp(x) / inv_std32 + mean32: inv_std32 is off by 4 u relatively (norm_bound), the division and the sum round once each,
    the mean's fp32 image is off by u |mean|."""
    mean, var, _ = state
    scaled = np.abs(np.clip(raw, -5.0, 5.0)) * math.sqrt(var + eps)
    return U32 * (5.0 * scaled + abs(mean) + np.abs(R.rms_denorm(raw, state, eps)))


def _checked_epoch(torch, tr, worst):
    """One epoch by train_epoch()'s steps, every product of collect(), _episodes() and prepare() compared with the fp64 restatement."""
    cfg, col, H, A = tr.cfg, tr.col, tr.cfg.horizon_length, tr.num_actions
    total = H * tr.rows
    raw = []
    inner = col.collect

    def collect_and_keep():                                   # the network's (normalised) value column, before collect() rewrites it
        inner()
        raw.append(col.values.clone())
        return col
    col.collect = collect_and_keep
    try:
        state0 = _rms_state(tr.value_rms) if tr.value_rms is not None else None
        tr.collect()
    finally:
        del col.collect
    torch.cuda.synchronize()
    rew, done, val = _np(col.rewards), _np(col.dones), _np(col.values)
    keep = lambda k, r: worst.__setitem__(k, max(worst.get(k, 0.0), r))
    if state0 is not None:
        want = R.rms_denorm(_np(raw[0]), state0)
        err, bound = np.abs(val - want), _denorm_bound(_np(raw[0]).astype(np.float64), state0)
        keep("denorm", _report("de-normalised values", err, bound))
        assert (err <= bound).all()
    else:
        assert torch.equal(raw[0], col.values)
    g = R.gae_loop(rew, val, done, cfg.gamma, cfg.tau, cfg.reward_scale)          # on the values the device holds now
    for name, got, want in (("advantages", col.advantages, g["adv"]), ("returns", col.returns, g["ret"])):
        err = np.abs(_np(got) - want)
        keep("gae", _report(f"GAE {name}", err, g["bound"]))
        assert (err <= g["bound"]).all(), name
    # the episode statistics, with the state carried in from the epochs before
    ep0 = (_np(tr.ep_ret).astype(np.float64), _np(tr.ep_len).astype(np.float64))
    out = _np(tr._episodes()).astype(np.float64)
    e = R.episodes_loop(rew, done, ep0[0], ep0[1], worst.setdefault("_ep_err", np.zeros(tr.rows)))
    worst["_ep_err"] = e["ep_err"]
    assert out[1] == e["sum_len"] and out[2] == e["count"]
    assert abs(out[0] - e["sum_ret"]) <= e["bound"] + U32 * abs(e["sum_ret"]), (out[0], e["sum_ret"], e["bound"])
    assert np.array_equal(_np(tr.ep_len), e["ep_len"])
    assert (np.abs(_np(tr.ep_ret) - e["ep_ret"]) <= e["ep_err"] + U32 * np.abs(e["ep_ret"])).all()
    print(f"  episodes finished {e['count']}: return sum error {abs(out[0] - e['sum_ret']):.3g}, bound {e['bound']:.3g}")
    # prepare()
    state1 = _rms_state(tr.value_rms) if tr.value_rms is not None else None
    assert state1 == state0
    tr.prepare()
    torch.cuda.synchronize()
    act, mu = _np(col.actions).reshape(total, A), _np(col.head[:H]).reshape(total, A + 1)[:, :A]
    v, r, adv = val[:H].reshape(total), _np(col.returns).reshape(total), _np(col.advantages).reshape(total)
    ref = R.prepare_reference(act, mu, _np(col.sigma), v, r, adv, rms_state=state1, normalize_advantage=cfg.normalize_advantage)
    bounds = dict(old_nlp=nlp_bound(ref, A))
    bounds["adv"] = adv_bound(adv, total) if cfg.normalize_advantage else np.zeros(total)
    if state1 is not None:
        bounds["old_v"], bounds["ret"] = norm_bound(v, R.rms_merge(state1, v)), norm_bound(r, ref["rms_state"])
        got = _rms_state(tr.value_rms)
        print(f"  value statistics: device {got}, fp64 {tuple(float(x) for x in ref['rms_state'])}")
        # rtol 1e-9 as test_policy_backward has it; the mean's absolute term on the scale of the data's spread (a mean may sit near zero)
        np.testing.assert_allclose(got[0], ref["rms_state"][0], rtol=1e-9, atol=1e-9 * math.sqrt(ref["rms_state"][1]))
        np.testing.assert_allclose(got[1], ref["rms_state"][1], rtol=1e-9, atol=0)
        assert got[2] == ref["rms_state"][2]
    else:
        bounds["old_v"], bounds["ret"] = np.zeros(total), np.zeros(total)
    for k, bound in bounds.items():
        err = np.abs(_np(getattr(tr, k)).astype(np.float64) - ref[k])
        bound = bound + U32 * np.abs(ref[k]) * (bound > 0)                         # the fp32 result's own rounding; plain copies: equal
        keep(k, _report(f"prepare {k}", err, bound))
        assert (err <= bound).all(), k
    tr.learn()
    col.sigma.copy_(torch.exp(tr.logstd))
    col.next_horizon()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("task", ["HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"])
def test_collect_and_prepare_match_fp64_on_real_rollouts(torch_cuda, task, normalize):
    """Two epochs, so the second starts from value statistics, a log-std and carried episodes that are no longer the initial ones."""
    torch = torch_cuda
    import isaacgym_amd
    from isaacgym_amd import ppo
    num_envs = 256
    t = isaacgym_amd.make(seed=5, task=task, num_envs=num_envs)
    tr = ppo.PPOTrainer(t, ppo.PPOConfig(minibatch_size=8192, normalize_value=normalize, normalize_advantage=normalize), seed=5)
    if task == "Humanoid12PingpongTiltG1":
        assert tr.rows == 2 * num_envs
    assert (tr.value_rms is not None) == normalize
    worst = {}
    for epoch in range(2):
        print(f"{task} normalize={normalize} epoch {epoch}")
        _checked_epoch(torch, tr, worst)
    print("worst error / bound:", {k: round(v, 4) for k, v in worst.items() if not k.startswith("_")})


# ======================================================================================================================================
# 2. the loss kernel: ragged and tiny batches, the action widths' ends, every switch, the workspace, wide strides
# ======================================================================================================================================
MARGIN = 1e-3


def _edge_batch(rng, m, a):
    """test_ppo_gpu._batch's rows (log ratio in {+-0.6, +-0.05, 0} +- 0.02, v - old_v in {+-0.5, +-0.1}), with the returns placed so that the
    third discontinuous switch of the value gradient — (v - r)^2 against (vc - r)^2 where the clamp is active, which meets at r = (v + vc) / 2
    — is at least 0.05 away as well."""
    from test_ppo_gpu import _batch
    b = _batch(rng, m, a)
    v, ov = b["value"].astype(np.float64), b["old_values"].astype(np.float64)
    vc = ov + np.clip(v - ov, -0.2, 0.2)
    b["returns"] = (0.5 * (v + vc) + rng.choice([-1.0, 1.0], m) * rng.uniform(0.05, 2.0, m)).astype(np.float32)
    return b


def _assert_margins(b, e_clip, m):
    """On the fp64 reference's own quantities: no row within MARGIN of a switch; both sides of each present from 64 rows on."""
    from isaacgym_amd import ppo
    f = lambda k: b[k].astype(np.float64)
    ls = f("logstd")
    z = (f("actions") - f("mu")) / np.exp(ls)
    ratio = np.exp(f("old_neglogp") - (0.5 * (z * z).sum(1) + ppo.HALF_LOG_2PI * z.shape[1] + ls.sum()))
    d = f("value") - f("old_values")
    vc = f("old_values") + np.clip(d, -e_clip, e_clip)
    gap = np.abs(np.abs(f("value") - f("returns")) - np.abs(vc - f("returns")))[np.abs(d) > e_clip]
    assert np.abs(ratio - (1 + e_clip)).min() > MARGIN and np.abs(ratio - (1 - e_clip)).min() > MARGIN
    assert np.abs(np.abs(d) - e_clip).min() > MARGIN
    assert gap.size == 0 or gap.min() > MARGIN
    if m >= 64:
        assert (ratio > 1 + e_clip).any() and (ratio < 1 - e_clip).any() and ((ratio > 1 - e_clip) & (ratio < 1 + e_clip)).any()
        assert (np.abs(d) > e_clip).any() and (np.abs(d) < e_clip).any()
        cu, cc = (f("value") - f("returns")) ** 2, (vc - f("returns")) ** 2
        assert (cu > cc).any() and (cu < cc).any()
        assert (np.abs(f("mu")) > 1.1).any()


def _device_batch(torch, b, a):
    """The batch as the trainer holds it: mu | value in one [m, a + 1] head buffer, old mu in another."""
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    m = b["mu"].shape[0]
    head, old_head = torch.zeros((m, a + 1), device="cuda"), torch.zeros((m, a + 1), device="cuda")
    head[:, :a], head[:, a], old_head[:, :a] = d(b["mu"]), d(b["value"]), d(b["old_mu"])
    return (head[:, :a], head[:, a:], d(b["actions"]), old_head[:, :a], d(b["old_sigma"]), d(b["old_neglogp"]), d(b["advantages"]),
            d(b["old_values"]), d(b["returns"]), d(b["logstd"]))


def _launch(torch, lg, args, scale):
    """-> (d_head, d_logstd, stats) of one call, cloned."""
    stats = torch.full((8,), -7.0, device="cuda")
    dh = lg(*args, torch.full((1,), scale, device="cuda"), stats).clone()
    return dh, lg.d_logstd.clone(), stats


def _compare_loss(out, ref, a, what):
    """The existing tolerances of test_ppo_gpu.test_loss_kernel_matches_fp64; -> the worst error in units of its tolerance."""
    from isaacgym_amd import ppo
    dh, dls, stats = (_np(t).astype(np.float64) for t in out)
    worst = 0.0
    for got, want, name in ((dh[:, :a], ref["d_mu"], "d mu"), (dh[:, a], ref["d_value"], "d value"), (dls, ref["d_logstd"], "d logstd")):
        tol = 1e-5 * np.abs(want).max() + 1e-5 * np.abs(want)
        worst = max(worst, float((np.abs(got - want) / np.where(tol > 0, tol, 1.0)).max()))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max(), err_msg=f"{what}: {name}")
    for i, k in enumerate(ppo.STATS):
        worst = max(worst, abs(stats[i] - ref[k]) / (1e-6 + 1e-5 * abs(ref[k])))
        np.testing.assert_allclose(stats[i], ref[k], rtol=1e-5, atol=1e-6, err_msg=f"{what}: {k}")
    assert stats[7] == 0.0
    return worst


SWITCHES = [(cv, ec, sc) for cv in (True, False) for ec in (0.0, 0.01) for sc in (1.0, 65536.0)]


@pytest.mark.parametrize("a", [1, 4, 7, 27, 32])
@pytest.mark.parametrize("m", [1, 63, 64, 255, 256, 257, 1000, 8192 + 64])
def test_loss_kernel_shapes_and_switches(torch_cuda, m, a):
    """Ragged batches (m not a multiple of 64): every combination of clip_value, entropy_coef and scale; the others: the two opposite corners."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    rng = np.random.default_rng(1000 * m + a)
    b = _edge_batch(rng, m, a)
    _assert_margins(b, 0.2, m)
    args = _device_batch(torch, b, a)
    worst = 0.0
    for clip_value, entropy_coef, scale in (SWITCHES if m % 64 else [SWITCHES[1], SWITCHES[6]]):
        cfg = ppo.PPOConfig(entropy_coef=entropy_coef, clip_value=clip_value)
        ref = ppo.loss_grad_reference(**b, e_clip=cfg.e_clip, critic_coef=cfg.critic_coef, bounds_loss_coef=cfg.bounds_loss_coef,
                                      entropy_coef=entropy_coef, clip_value=clip_value, scale=scale)
        lg = ppo.LossGrad(a, m, "cuda", cfg)
        first, second = _launch(torch, lg, args, scale), _launch(torch, lg, args, scale)
        torch.cuda.synchronize()
        worst = max(worst, _compare_loss(first, ref, a, f"clip_value={clip_value} entropy_coef={entropy_coef} scale={scale}"))
        for x, y in zip(first, second):                               # no float atomics: bitwise reproducible
            assert torch.equal(x, y)
    print(f"  m={m} a={a}: worst error {worst:.3g} of the tolerance (rtol 1e-5, atol 1e-5 x max; stats rtol 1e-5, atol 1e-6)")


@pytest.mark.parametrize("a", [7, 32])
def test_loss_workspace_reused_after_a_larger_batch(torch_cuda, a):
    """One LossGrad sized for 8192 + 64 rows: a call at that size, then one at 63 rows, which must equal a fresh object's result bitwise
    (the partial rows and d_head rows the larger call left behind are not read)."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    big, small = 8192 + 64, 63
    rng = np.random.default_rng(a)
    cfg = ppo.PPOConfig(entropy_coef=0.01)
    b_big, b_small = _edge_batch(rng, big, a), _edge_batch(rng, small, a)
    lg = ppo.LossGrad(a, big, "cuda", cfg)
    _launch(torch, lg, _device_batch(torch, b_big, a), 65536.0)
    assert float(lg.partial.abs().max()) > 0
    args = _device_batch(torch, b_small, a)
    reused = _launch(torch, lg, args, 65536.0)
    fresh = _launch(torch, ppo.LossGrad(a, small, "cuda", cfg), args, 65536.0)
    torch.cuda.synchronize()
    for x, y in zip(reused, fresh):
        assert x.shape == y.shape and torch.equal(x, y)
    ref = ppo.loss_grad_reference(**b_small, e_clip=cfg.e_clip, critic_coef=cfg.critic_coef, bounds_loss_coef=cfg.bounds_loss_coef,
                                  entropy_coef=cfg.entropy_coef, clip_value=True, scale=65536.0)
    print(f"  a={a}: worst error {_compare_loss(reused, ref, a, 'reused workspace'):.3g} of the tolerance")


@pytest.mark.parametrize("m,a", [(257, 1), (1000, 27), (63, 32), (8192 + 64, 32)])
def test_loss_kernel_wide_row_strides(torch_cuda, m, a):
    """ppenv_ppo_loss_grad through its argument struct with every row stride larger than needed: columns 0 .. a of d_head equal the packed
    call's bitwise, every other column keeps its sentinel."""
    torch = torch_cuda
    from isaacgym_amd import _lib, ppo
    rng = np.random.default_rng(m + a)
    b = _edge_batch(rng, m, a)
    _assert_margins(b, 0.2, m)
    cfg = ppo.PPOConfig(entropy_coef=0.01)
    scale, sentinel = 65536.0, 12345.0
    packed = _launch(torch, ppo.LossGrad(a, m, "cuda", cfg), _device_batch(torch, b, a), scale)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def wide(x, ld, col=0):
        x = x.reshape(m, -1)
        buf = torch.full((m, ld), sentinel, device="cuda")
        buf[:, col:col + x.shape[1]] = d(x)
        return buf
    ld_mu, ld_value, ld_act, ld_old, ld_dh = a + 5, 3, a + 3, a + 2, a + 1 + 6
    mu, value, act, old_mu = wide(b["mu"], ld_mu), wide(b["value"], ld_value), wide(b["actions"], ld_act), wide(b["old_mu"], ld_old)
    vec = {k: d(b[k]) for k in ("old_sigma", "old_neglogp", "advantages", "old_values", "returns", "logstd")}
    L = _lib.lib()
    partial = torch.zeros(int(L.ppenv_ppo_loss_partial_floats(m)), device="cuda")
    sc = torch.full((1,), scale, device="cuda")
    outs = []
    for _ in range(2):
        d_head, d_logstd, stats = torch.full((m, ld_dh), sentinel, device="cuda"), torch.zeros(a, device="cuda"), torch.zeros(8, device="cuda")
        p = ppo.PPOLossArgs(m, a, mu.data_ptr(), ld_mu, value.data_ptr(), ld_value, act.data_ptr(), ld_act, old_mu.data_ptr(), ld_old,
                            vec["old_sigma"].data_ptr(), vec["old_neglogp"].data_ptr(), vec["advantages"].data_ptr(), vec["old_values"].data_ptr(),
                            vec["returns"].data_ptr(), vec["logstd"].data_ptr(), cfg.e_clip, cfg.critic_coef, cfg.bounds_loss_coef, ppo.SOFT_BOUND,
                            cfg.entropy_coef, 1, sc.data_ptr(), d_head.data_ptr(), ld_dh, d_logstd.data_ptr(), stats.data_ptr(), partial.data_ptr())
        _lib.check(L.ppenv_ppo_loss_grad(C.byref(p), torch.cuda.current_stream().cuda_stream))
        outs.append((d_head, d_logstd, stats))
    torch.cuda.synchronize()
    d_head, d_logstd, stats = outs[0]
    assert torch.equal(d_head[:, :a + 1], packed[0]) and torch.equal(d_logstd, packed[1]) and torch.equal(stats, packed[2])
    assert bool((d_head[:, a + 1:] == sentinel).all())
    for t in (mu[:, a:], value[:, 1:], act[:, a:], old_mu[:, a:]):                    # the inputs' padding was neither needed nor written
        assert bool((t == sentinel).all())
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y)
    ref = ppo.loss_grad_reference(**b, e_clip=cfg.e_clip, critic_coef=cfg.critic_coef, bounds_loss_coef=cfg.bounds_loss_coef,
                                  entropy_coef=cfg.entropy_coef, clip_value=True, scale=scale)
    print(f"  m={m} a={a}: worst error {_compare_loss((d_head[:, :a + 1], d_logstd, stats), ref, a, 'wide strides'):.3g} of the tolerance")


# ======================================================================================================================================
# 3. DeviceAdam: layouts, launch shapes, the table's limit, a constant scale, a long run
# ======================================================================================================================================
N_ELEMS = 2520                                              # 63 x 40 = 60 x 42
LAYOUTS = ["aligned", "offset1", "cols42", "padded4", "padded_odd"]
P_PAD, G_PAD = 777.0, float("inf")                          # what the padding holds: the norm must not see it, the step must not touch it


def _layout(torch, kind, p_values):
    """The same 2520 values as one matrix in a layout that takes the kernels' vector path (aligned, padded4) or their element path (a
    pointer one element into its storage, 42 columns, a gradient row stride of 43 under a padded parameter).
    -> (p view, g view, p storage, g storage, masks of the storages' padding)."""
    rows, cols = (60, 42) if kind == "cols42" else (63, 40)
    ld_p, ld_g, off = {"aligned": (cols, cols, 0), "offset1": (cols, cols, 1), "cols42": (cols, cols, 0), "padded4": (48, 44, 0),
                       "padded_odd": (48, 43, 0)}[kind]

    def make(ld, pad):
        store = torch.full((off + rows * ld,), pad, device="cuda")
        view = store[off:].view(rows, ld)[:, :cols]
        mask = torch.ones_like(store, dtype=torch.bool)
        mask[off:].view(rows, ld)[:, :cols] = False
        return store, view, mask
    ps, p, pmask = make(ld_p, P_PAD)
    gs, g, gmask = make(ld_g, G_PAD)
    p.copy_(p_values.view(rows, cols))
    vector = cols % 4 == 0 and ld_p % 4 == 0 and ld_g % 4 == 0 and p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    assert vector == (kind in ("aligned", "padded4")), (kind, p.data_ptr() % 16, g.data_ptr() % 16)
    return p, g, ps, gs, pmask, gmask


def _torch_adam(torch, params, lr):
    tp = [torch.nn.Parameter(p.detach().double().cpu().clone()) for p in params]
    return tp, torch.optim.Adam(tp, lr=lr, eps=1e-8, foreach=False)


def _assert_adam_close(torch, opt, params, tp, topt, what):
    """The tolerances of test_ppo_gpu.test_clip_adam_matches_torch; -> worst error in units of them."""
    worst = 0.0
    for i, (p, q) in enumerate(zip(params, tp)):
        q, st = q.detach(), topt.state[tp[i]]
        for mine, theirs, rtol, atol, name in ((p, q, 1e-6, 1e-7, "parameter"), (opt.exp_avg[i], st["exp_avg"], 1e-6, 1e-6, "exp_avg"),
                                               (opt.exp_avg_sq[i], st["exp_avg_sq"], 1e-6, 1e-6, "exp_avg_sq")):
            mine = mine.detach().double().cpu()
            tol = atol * float(theirs.abs().max()) + rtol * theirs.abs()
            worst = max(worst, float(((mine - theirs).abs() / tol).max()))
            torch.testing.assert_close(mine, theirs, rtol=rtol, atol=atol * float(theirs.abs().max()), msg=f"{what}: {name} {i}")
    return worst


def test_adam_layouts_agree_bitwise_and_match_torch(torch_cuda):
    """The same values and gradients in five layouts, 5 steps each with truncate=False: every layout within the existing tolerances of torch's
    fp64 Adam, the padding untouched and unseen by the norm, and parameters and moments bitwise equal across layouts.  (This found the vector
    and the element loop fusing the second moment's products differently; adam1 in csrc/ppenv_ppo.hip now spells its roundings out.)"""
    torch = torch_cuda
    from isaacgym_amd import ppo
    gen = torch.Generator().manual_seed(3)
    p0, v0 = torch.randn(N_ELEMS, generator=gen).cuda(), torch.randn(27, generator=gen).cuda()
    scale, lr, steps = 1024.0, 1e-3, 5
    grads = [(torch.randn(N_ELEMS, generator=gen) * 1e-2, torch.randn(27, generator=gen) * 1e-2) for _ in range(steps)]
    results = {}
    for kind in LAYOUTS:
        p, g, ps, gs, pmask, gmask = _layout(torch, kind, p0)
        vec, gvec = v0.clone(), torch.zeros(27, device="cuda")
        opt = ppo.DeviceAdam([p, vec], [g, gvec], lr, max_norm=10.0, truncate=False, init_scale=scale, growth_interval=2000)
        tp, topt = _torch_adam(torch, [p, vec], lr)
        worst = 0.0
        for gm, gv in grads:
            g.copy_((gm * scale).cuda().view(g.shape))
            gvec.copy_((gv * scale).cuda())
            tp[0].grad, tp[1].grad = gm.double().view(g.shape), gv.double()
            topt.step()
            opt.step()
            worst = max(worst, _assert_adam_close(torch, opt, [p, vec], tp, topt, kind))
        f = {k: float(v) for k, v in opt.fields().items()}
        want_norm = math.sqrt(float((grads[-1][0].double() ** 2).sum() + (grads[-1][1].double() ** 2).sum()))
        print(f"  {kind}: worst error {worst:.3g} of the tolerance; grad_norm {f['grad_norm']:.9g} (fp64 {want_norm:.9g})")
        assert (f["step"], f["skipped"], f["scale"]) == (steps, 0, scale)          # the inf in the gradient's padding was not summed
        assert abs(f["grad_norm"] - want_norm) <= 1e-6 * want_norm
        assert bool((ps[pmask] == P_PAD).all()) and bool((gs[gmask] == G_PAD).all())
        results[kind] = [t.detach().reshape(-1).clone() for t in (p, opt.exp_avg[0], opt.exp_avg_sq[0], vec, opt.exp_avg[1], opt.exp_avg_sq[1])]
    for kind in LAYOUTS[1:]:                                   # truncate=False: the element arithmetic does not depend on the norm
        for x, y, name in zip(results["aligned"], results[kind], ("p", "exp_avg", "exp_avg_sq", "vector p", "vector exp_avg", "vector exp_avg_sq")):
            assert torch.equal(x, y), (kind, name)


@pytest.mark.parametrize("truncate", [False, True])
def test_adam_launch_shapes(torch_cuda, truncate):
    """parts workgroups, from one to more than the 256 lanes that sum the slab.  truncate=False: parameters bitwise equal across parts;
    truncate=True with an active clip: the norm against fp64 (rtol 1e-6: one fp32 rounding of an fp64 sum) and the parameters against torch."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    gen = torch.Generator().manual_seed(8)
    shapes = [(63, 40), (60, 42), (27,), (300, 64)]
    p0 = [torch.randn(s, generator=gen) for s in shapes]
    scale, lr, steps, max_norm = 1024.0, 1e-3, 3, 10.0
    grads = [[torch.randn(s, generator=gen) * (0.2 if truncate else 1e-2) for s in shapes] for _ in range(steps)]
    results = {}
    for parts in (1, 7, 256, 512, 1000):
        params, gbufs = [p.clone().cuda() for p in p0], [torch.zeros(s, device="cuda") for s in shapes]
        opt = ppo.DeviceAdam(params, gbufs, lr, max_norm=max_norm, truncate=truncate, init_scale=scale, growth_interval=2000, parts=parts)
        assert opt.slab.numel() == parts
        tp, topt = _torch_adam(torch, params, lr)
        worst = 0.0
        for gs in grads:
            for buf, q, g in zip(gbufs, tp, gs):
                buf.copy_((g * scale).cuda())
                q.grad = g.double().clone()
            want_norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
            if truncate:
                assert want_norm > max_norm                      # the clip is active
                torch.nn.utils.clip_grad_norm_(tp, max_norm)
            topt.step()
            opt.step()
            got_norm = float(opt.fields()["grad_norm"])
            assert abs(got_norm - want_norm) <= 1e-6 * want_norm, (parts, got_norm, want_norm)
            worst = max(worst, _assert_adam_close(torch, opt, params, tp, topt, f"parts={parts}"))
        print(f"  truncate={truncate} parts={parts}: worst error {worst:.3g} of the tolerance; grad_norm {got_norm:.9g} (fp64 {want_norm:.9g})")
        assert int(opt.fields()["step"]) == steps and int(opt.fields()["skipped"]) == 0
        results[parts] = [p.clone() for p in params] + [t.clone() for t in opt.exp_avg + opt.exp_avg_sq]
    if not truncate:
        for parts in (7, 256, 512, 1000):
            for x, y in zip(results[1], results[parts]):
                assert torch.equal(x, y), parts


def test_adam_table_of_64_tensors_and_the_refusal_of_65(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd import _lib, ppo
    gen = torch.Generator().manual_seed(13)
    scale, lr = 1024.0, 1e-3
    items = [_layout(torch, LAYOUTS[i % len(LAYOUTS)], torch.randn(N_ELEMS, generator=gen).cuda()) for i in range(64)]
    params, gbufs = [it[0] for it in items], [it[1] for it in items]
    opt = ppo.DeviceAdam(params, gbufs, lr, max_norm=10.0, truncate=True, init_scale=scale, growth_interval=2000)
    tp, topt = _torch_adam(torch, params, lr)
    worst = 0.0
    for step in range(3):
        for buf, q in zip(gbufs, tp):
            g = torch.randn(buf.shape, generator=gen) * 0.05
            buf.copy_((g * scale).cuda())
            q.grad = g.double()
        norm = float(torch.nn.utils.clip_grad_norm_(tp, 10.0))
        assert norm > 10.0
        topt.step()
        opt.step()
        assert abs(float(opt.fields()["grad_norm"]) - norm) <= 1e-6 * norm
        worst = max(worst, _assert_adam_close(torch, opt, params, tp, topt, f"step {step}"))
    print(f"  64 tensors: worst error {worst:.3g} of the tolerance")
    assert int(opt.fields()["step"]) == 3 and int(opt.fields()["skipped"]) == 0
    for _, _, ps, gs, pmask, gmask in items:
        assert bool((ps[pmask] == P_PAD).all()) and bool((gs[gmask] == G_PAD).all())
    # 65: refused by the class, and by both entry points before any device call (the table pointer is the valid one of 64)
    with pytest.raises(AssertionError):
        ppo.DeviceAdam(params + [torch.zeros(4, device="cuda")], gbufs + [torch.zeros(4, device="cuda")], lr)
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    before = [p.clone() for p in params] + [opt.state.clone()]
    assert L.ppenv_ppo_grad_sumsq(opt.table.data_ptr(), 65, opt.slab.data_ptr(), opt.parts, st) == PPENV_EINVAL
    assert b"64 tensors" in L.ppenv_last_error()
    assert L.ppenv_ppo_adam_step(opt.table.data_ptr(), 65, opt.slab.data_ptr(), opt.parts, opt.hp, opt.lr.data_ptr(), opt.state[0].data_ptr(),
                                 opt.state[1].data_ptr(), st) == PPENV_EINVAL
    torch.cuda.synchronize()
    for x, y in zip(before, params + [opt.state]):
        assert torch.equal(x, y)


def test_adam_constant_scale(torch_cuda):
    """dynamic=False (mixed_precision: False): scale 1 and factors 1.0 — a non-finite gradient skips the step and leaves the scale at 1, clean
    steps never change it, and the arithmetic is torch's."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    gen = torch.Generator().manual_seed(21)
    shapes = [(63, 40), (60, 42), (27,)]
    params, gbufs = [torch.randn(s, generator=gen).cuda() for s in shapes], [torch.zeros(s, device="cuda") for s in shapes]
    opt = ppo.DeviceAdam(params, gbufs, 1e-3, max_norm=10.0, truncate=True, init_scale=1.0, growth_interval=3, dynamic=False)
    tp, topt = _torch_adam(torch, params, 1e-3)
    read = lambda: {k: float(v) for k, v in opt.fields().items()}
    worst, clean = 0.0, 0
    for step in range(9):
        for buf, q in zip(gbufs, tp):
            g = torch.randn(buf.shape, generator=gen) * 1e-2
            buf.copy_(g.cuda())
            q.grad = g.double()
        bad = {2: float("inf"), 5: float("nan")}.get(step)
        if bad is not None:
            gbufs[1][7, 5] = bad                              # an injected value in a gradient buffer
            before = [t.clone() for t in params + opt.exp_avg + opt.exp_avg_sq]
        else:
            torch.nn.utils.clip_grad_norm_(tp, 10.0)
            topt.step()
            clean += 1
        opt.step()
        s = read()
        assert s["scale"] == 1.0 and s["step"] == clean and s["skipped"] == step + 1 - clean, (step, s)
        if bad is not None:
            for x, y in zip(before, params + opt.exp_avg + opt.exp_avg_sq):
                assert torch.equal(x, y)
        else:
            worst = max(worst, _assert_adam_close(torch, opt, params, tp, topt, f"step {step}"))
    print(f"  constant scale: worst error {worst:.3g} of the tolerance")


def test_adam_long_run_and_scale_growth(torch_cuda):
    """2100 steps with fresh gradients: the scale doubles exactly once, after the 2000th clean step, and the parameters follow torch's fp64
    Adam on the same unscaled gradients.  fp32 rounding accumulates over 2100 steps, so the tolerance is measured on a reference of the same
    precision: torch's own fp32 Adam (foreach=False, CPU) on the same gradients — its worst deviation from the fp64 run relative to max |p|;
    the kernel is allowed twice that (the same arithmetic; the bias corrections' constants are rounded in another order)."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    gen = torch.Generator().manual_seed(34)
    shapes = [(33, 40), (17, 27), (27,)]
    p0 = [torch.randn(s, generator=gen) for s in shapes]
    lr, steps, interval, init = 1e-3, 2100, 2000, 65536.0
    params, gbufs = [p.clone().cuda() for p in p0], [torch.zeros(s, device="cuda") for s in shapes]
    opt = ppo.DeviceAdam(params, gbufs, lr, max_norm=10.0, truncate=True, init_scale=init, growth_interval=interval)
    p64, o64 = _torch_adam(torch, p0, lr)
    p32 = [torch.nn.Parameter(p.clone()) for p in p0]
    o32 = torch.optim.Adam(p32, lr=lr, eps=1e-8, foreach=False)
    scales = []
    for step in range(steps):
        gs = [torch.randn(s, generator=gen) * 1e-2 for s in shapes]
        assert math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs)) < 10.0        # the clip stays inactive: the references do not clip
        for buf, a, b, g in zip(gbufs, p64, p32, gs):
            buf.copy_(g.cuda() * opt.scale)                    # a power of two: exact
            a.grad, b.grad = g.double(), g
        o64.step()
        o32.step()
        opt.step()
        scales.append(opt.fields()["scale"].clone())
    f = {k: float(v) for k, v in opt.fields().items()}
    assert (f["step"], f["skipped"]) == (steps, 0) and f["growth_tracker"] == steps - interval
    scales = torch.stack(scales).cpu().tolist()
    assert scales[:interval - 1] == [init] * (interval - 1) and scales[interval - 1:] == [2 * init] * (steps - interval + 1)
    dev32 = max(float((b.detach().double() - a.detach()).abs().max() / a.detach().abs().max()) for a, b in zip(p64, p32))
    devk = max(float((p.double().cpu() - a.detach()).abs().max() / a.detach().abs().max()) for a, p in zip(p64, params))
    print(f"  after {steps} steps, worst |p - p_fp64| / max |p|: torch fp32 {dev32:.3g}, the kernel {devk:.3g} (allowed {2 * dev32:.3g})")
    assert dev32 > 0 and devk <= 2 * dev32


# ======================================================================================================================================
# 4. RunningMeanStd where the trainer uses it: one column, horizon x rows rows, data far from zero
# ======================================================================================================================================
def _rms_data(rng, m, k, i):
    """Returns-like: magnitude 1e3, the mean three standard deviations from zero (the ratio the one-pass variance's fp64 cancellation allows at
    524 288 rows, see _check_rms), varying from batch to batch and column to column."""
    return (rng.normal(0.0, 1.0, (m, k)) * 1e3 * rng.uniform(0.9, 1.1, k) + 1e3 * (3.0 - 0.2 * i) * rng.uniform(0.9, 1.0, k)).astype(np.float32)


def _check_rms(torch, rms, state, x, what):
    """One update against the fp64 parallel-moments rule at the existing rtol 1e-9.  The kernel's one-pass variance (sum x^2 - m mean^2 in
    fp64) loses up to m 2^-53 mean^2 / var relatively to cancellation on its own: the data must leave that below the tolerance."""
    m = x.shape[0]
    x64 = x.astype(np.float64)
    cancel = float((m * 2.0 ** -53 * x64.mean(0) ** 2 / x64.var(0, ddof=1)).max())
    assert cancel < 1e-9, cancel
    rms.update(torch.from_numpy(x).cuda())
    state = R.rms_merge(state, x64)
    torch.cuda.synchronize()
    got = (_np(rms.running_mean), _np(rms.running_var), float(rms.count.cpu()))
    errs = [float(np.abs(got[i] / state[i] - 1.0).max()) for i in (0, 1)]
    print(f"  {what}: m={m} k={x.shape[1]}: mean rel. error {errs[0]:.3g}, var rel. error {errs[1]:.3g} (rtol 1e-9; cancellation bound {cancel:.3g})")
    np.testing.assert_allclose(got[0], state[0], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got[1], state[1], rtol=1e-9, atol=0)
    assert got[2] == state[2]
    mean32, var32 = state[0].astype(np.float32), state[1].astype(np.float32)
    np.testing.assert_allclose(_np(rms.mean), mean32, rtol=1e-6)
    np.testing.assert_allclose(_np(rms.inv_std), 1.0 / np.sqrt(var32 + np.float32(1e-5)), rtol=1e-6)
    return state


@pytest.mark.parametrize("m,k", [(131072, 1), (524288, 1), (131072 + 77, 1), (1000, 64), (1000, 65), (1000, 80)])
def test_running_mean_std_at_the_value_statistics_shapes(torch_cuda, m, k):
    torch = torch_cuda
    from isaacgym_amd.policy import RunningMeanStd
    rng = np.random.default_rng(m + k)
    rms = RunningMeanStd(k, "cuda:0")
    state = (np.zeros(k), np.ones(k), 1.0)
    for i in range(3):
        state = _check_rms(torch, rms, state, _rms_data(rng, m, k, i), f"update {i}")


def test_running_mean_std_changing_row_counts(torch_cuda):
    """One object: the workspace grows (zeroed tickets again) and is then used by a smaller batch (row blocks the larger one left are not read)."""
    torch = torch_cuda
    from isaacgym_amd.policy import RunningMeanStd
    rng = np.random.default_rng(9)
    rms = RunningMeanStd(1, "cuda:0")
    state = (np.zeros(1), np.ones(1), 1.0)
    for i, m in enumerate((131072, 524288, 131072 + 77, 1, 127)):
        x = _rms_data(rng, max(m, 2), 1, i % 3)[:m]
        if m == 1:                                           # one row: batch variance 0 by rl_games' m > 1 guard; no cancellation to bound
            rms.update(torch.from_numpy(x).cuda())
            state = R.rms_merge(state, x.astype(np.float64))
            np.testing.assert_allclose(_np(rms.running_var), state[1], rtol=1e-9, atol=0)
            np.testing.assert_allclose(_np(rms.running_mean), state[0], rtol=1e-9, atol=0)
        else:
            state = _check_rms(torch, rms, state, x, f"batch {i}")


# ======================================================================================================================================
# 5. GAE edges
# ======================================================================================================================================
GAE_SHAPES = [(1, 1), (1, 257), (32, 255), (32, 256), (32, 257), (5, 4096)]


def _gae_dones(torch, kind, rng, h, n):
    if kind == "none":
        d = np.zeros((h, n), dtype=np.int64)
    elif kind == "all":
        d = np.ones((h, n), dtype=np.int64)
    else:
        d = (rng.random((h, n)) < 0.2).astype(np.int64)
        if kind == "values":                                  # any non-zero int64 is a done: 2, and 2^32 (zero in its low 32 bits)
            d = d * rng.choice([2, 2 ** 32], (h, n))
    return d


@pytest.mark.parametrize("kind", ["none", "all", "random", "values"])
@pytest.mark.parametrize("h,n", GAE_SHAPES)
def test_gae_edges_match_the_fp64_recurrence(torch_cuda, h, n, kind):
    torch = torch_cuda
    from isaacgym_amd.collector import gae
    rng = np.random.default_rng(100 * h + n)
    rew = (rng.standard_normal((h, n)) * 50).astype(np.float32)
    head = rng.standard_normal((h + 1, n, 3)).astype(np.float32)
    done = _gae_dones(torch, kind, rng, h, n)
    dev_head = torch.from_numpy(head).cuda()
    adv, ret = gae(torch.from_numpy(rew).cuda(), dev_head[:, :, 2], torch.from_numpy(done).cuda(), 0.99, 0.95, 0.01)   # a strided column view
    torch.cuda.synchronize()
    want = R.gae_loop(rew, head[:, :, 2], done, 0.99, 0.95, 0.01)
    assert adv.shape == ret.shape == (h, n)
    for got, w, name in ((adv, want["adv"], "advantages"), (ret, want["ret"], "returns")):
        err = np.abs(_np(got) - w)
        print(f"  h={h} n={n} {kind} {name}: worst error {err.max():.3g} (atol 1e-5 + rtol 1e-5)")
        np.testing.assert_allclose(_np(got), w, rtol=1e-5, atol=1e-5, err_msg=name)
    # integer data, gamma = tau = reward_scale = 1: every fp32 operation is exact
    rew_i, head_i = rng.integers(-3, 5, (h, n)).astype(np.float32), rng.integers(-3, 5, (h + 1, n, 3)).astype(np.float32)
    dev_head = torch.from_numpy(head_i).cuda()
    adv, ret = gae(torch.from_numpy(rew_i).cuda(), dev_head[:, :, 2], torch.from_numpy(done).cuda(), 1.0, 1.0, 1.0)
    torch.cuda.synchronize()
    want = R.gae_loop(rew_i, head_i[:, :, 2], done, 1.0, 1.0, 1.0)
    assert np.array_equal(_np(adv).astype(np.float64), want["adv"]) and np.array_equal(_np(ret).astype(np.float64), want["ret"])
