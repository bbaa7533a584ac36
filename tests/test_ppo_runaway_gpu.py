"""The PPO minibatch tail on the MI355X where the policy has run away (seed 43 of the privileged-critic comparison: mu at +-20,
old_neglogp at 8e3, the fp16 gradients overflowing step after step): the loss gradient against fp64 at ratios of 0, denormal, huge and
inf; the fp32 -> fp16 cast of the head gradient at fp16's ends; DeviceAdam over the loss scale's whole range against the numpy restatement
of its bounded rule (ppo_reference.scaler_update; include/ppenv_ppo.h); and the pieces together through a burst of 160 overflowing
minibatches and a checkpoint whose scale had been halved to a denormal.  These are ordinary IEEE values through ordinary kernels.  Every
tolerance is an existing test's: test_ppo_gpu.test_loss_kernel_matches_fp64 (rtol 1e-5, atol 1e-5 x max |want|; statistics rtol 1e-5, atol
1e-6) and test_ppo_edges_gpu._assert_adam_close (test_clip_adam_matches_torch's)."""
import numpy as np
import pytest

import ppo_reference as R
from ppo_reference import CONSTANT, DYNAMIC, F32
from test_ppo_edges_gpu import _assert_adam_close, _device_batch, _launch, _np, _torch_adam, torch_cuda       # noqa: F401  (helpers, a fixture)

pytestmark = pytest.mark.gpu

DENORM_MIN = float(np.finfo(np.float32).smallest_subnormal)


def _bits(torch, t):
    """fp32 / fp16 as integers: NaNs compare equal to themselves, -0 differs from +0."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ======================================================================================================================================
# A. the loss gradient at runaway inputs
# ======================================================================================================================================
def _close_where_finite(got, want, atol, what):
    """Element-wise: non-finite exactly where the reference's fp32 image is, and within rtol 1e-5 + atol elsewhere.  -> worst error / tolerance."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    with np.errstate(over="ignore"):
        fin = np.isfinite(want.astype(F32))
    assert np.array_equal(np.isfinite(got), fin), f"{what}: non-finite at {np.flatnonzero(np.isfinite(got) != fin)}, reference {want}"
    if not fin.any():
        return 0.0
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5, atol=atol, err_msg=what)
    return float((np.abs(got[fin] - want[fin]) / (atol + 1e-5 * np.abs(want[fin]))).max())


@pytest.mark.parametrize("clip_value", [True, False])
@pytest.mark.parametrize("m,a", R.RUNAWAY_CASES)
def test_loss_kernel_at_runaway_inputs_matches_fp64(torch_cuda, m, a, clip_value):
    """Reference: ppo.loss_grad_reference with the ratio rounded to fp32 (ppo_reference.loss_grad_reference_f32_ratio); a row is non-finite
    where the fp32 image of the reference's d_mu / d_value is (the kernel writes fp32).  On top of the tolerance over all finite rows — whose
    atol, 1e-5 of a largest gradient near 1e38, is met by anything on the rows of a moderate ratio — those rows are compared again under
    the atol of their own largest gradient."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    b, cfg, ref, bad = R.runaway_case(m, a, clip_value)
    R.assert_runaway_margins(b, cfg.e_clip)
    print(f"  m={m} a={a} clip_value={clip_value}: finite rows {(~bad).mean():.3f}, non-finite rows {bad.mean():.3f}")
    assert (~bad).mean() >= 0.10 and bad.mean() >= 0.05
    lg = ppo.LossGrad(a, m, "cuda", cfg)
    args = _device_batch(torch, b, a)
    first, second = _launch(torch, lg, args, R.RUNAWAY_SCALE), _launch(torch, lg, args, R.RUNAWAY_SCALE)
    torch.cuda.synchronize()
    dh, dls, stats = (_np(t).astype(np.float64) for t in first)
    got_bad = ~np.isfinite(dh).all(1)
    assert np.array_equal(got_bad, bad), f"non-finite rows: the kernel's {np.flatnonzero(got_bad)}, the reference's {np.flatnonzero(bad)}"
    ok = ~bad
    moderate = ok & (np.abs(R.log_ratio(b)) < 1.0)
    assert moderate.sum() >= m // 8
    for rows, which in ((ok, "finite rows"), (moderate, "rows of a moderate ratio")):
        for got, want, name in ((dh[rows, :a], ref["d_mu"][rows], "d mu"), (dh[rows, a], ref["d_value"][rows], "d value")):
            atol = 1e-5 * np.abs(want).max()
            worst = float((np.abs(got - want) / (atol + 1e-5 * np.abs(want))).max())
            print(f"    {name}, {int(rows.sum())} {which}: worst error {worst:.3g} of the tolerance (max |want| {np.abs(want).max():.3g})")
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=atol, err_msg=f"{name}, {which}")
    fin = np.isfinite(ref["d_logstd"].astype(F32))
    worst = _close_where_finite(dls, ref["d_logstd"], 1e-5 * np.abs(ref["d_logstd"][fin]).max() if fin.any() else 0.0, "d logstd")
    for i, k in enumerate(ppo.STATS):
        worst = max(worst, _close_where_finite(stats[i], ref[k], 1e-6, k))
    print(f"    d logstd and statistics: worst error {worst:.3g} of the tolerance; loss {stats[0]}, a_loss {stats[1]}")
    assert stats[7] == 0.0
    for x, y in zip(first, second):                               # no float atomics: bitwise reproducible, NaNs included
        assert torch.equal(_bits(torch, x), _bits(torch, y))


# ======================================================================================================================================
# B. the head gradient's cast to fp16
# ======================================================================================================================================
SPECIALS = [65504.0, -65504.0, 65520.0, -65520.0, 1e5, -1e5, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 0.0, -0.0, float("inf"),
            -float("inf"), float("nan")]


@pytest.mark.parametrize("a", [7, 27])
def test_head_gradient_cast_is_torch_half_bitwise(torch_cuda, a):
    """What NativeMLPLearner.backward does first: prepare_input(dhead16, d_head) without statistics, 70 rows — the 64 rows the loss kernel
    writes at runaway inputs (finite, beyond fp16, inf, NaN) and six of hand-placed values: fp16's largest number, the first that rounds to
    inf, the smallest denormal, the tie below it that rounds to 0, both zeros, the infinities, a NaN."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    from isaacgym_amd.policy import prepare_input
    b, cfg, _, bad = R.runaway_case(64, a, True)
    d_head = torch.zeros((70, a + 1), device="cuda")
    d_head[:64] = ppo.LossGrad(a, 64, "cuda", cfg)(*_device_batch(torch, b, a), torch.full((1,), R.RUNAWAY_SCALE, device="cuda"),
                                                   torch.zeros(8, device="cuda"))
    n = 6 * (a + 1)
    d_head[64:] = torch.tensor([SPECIALS[i % len(SPECIALS)] for i in range(n)], dtype=torch.float32).view(6, a + 1).cuda()
    nh = (a + 1 + 7) // 8 * 8                                      # NativeMLPLearner.nh: whole 16-byte chunks
    out = torch.full((70, nh), 7.0, dtype=torch.float16, device="cuda")
    prepare_input(out, d_head)
    torch.cuda.synchronize()
    src = d_head.cpu()
    want, got = src.half(), out.cpu()
    assert bool(torch.isnan(src).any()) and bool(torch.isinf(src[:64]).any()) and bool((src[:64].abs() > 65520).any())
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got[:, :a + 1]), nan)
    differ = (_bits(torch, got[:, :a + 1]) != _bits(torch, want)) & ~nan
    assert not bool(differ.any()), (src[differ][:8], got[:, :a + 1][differ][:8], want[differ][:8])
    assert bool((_bits(torch, got[:, a + 1:]) == 0).all())         # the pad columns: +0
    print(f"  a={a}: {int(torch.isinf(want).sum())} inf, {int(nan.sum())} NaN, {int((want == 0).sum())} zeros of {want.numel()}; {nh - a - 1} pad columns")


# ======================================================================================================================================
# C. DeviceAdam over the scale's whole range
# ======================================================================================================================================
SHAPES = [(63, 40), (60, 42), (27,)]


def _adam(torch, seed=55, **kw):
    """Three small tensors, the first with a strided gradient (as test_ppo_gpu.test_nonfinite_gradient_skips_the_step has it), growth_interval 3.
    -> (DeviceAdam, params, gradient buffers, the initial values on the host)."""
    from isaacgym_amd import ppo
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(s, generator=gen) for s in SHAPES]
    params = [p.clone().cuda() for p in p0]
    gbufs = [torch.zeros(63, 48, device="cuda")[:, :40], torch.zeros(60, 42, device="cuda"), torch.zeros(27, device="cuda")]
    opt = ppo.DeviceAdam(params, gbufs, 1e-3, max_norm=10.0, truncate=True, growth_interval=3, **kw)
    return opt, params, gbufs, p0


def _set_scale(torch, opt, s0):
    """Both state rows, as load_state_dict leaves them; by bits, so that a denormal arrives as it is."""
    opt.state[:, 0] = int(np.array(s0, dtype=np.float32).view(np.int32))


def _record(opt):
    return {k: v.clone() for k, v in opt.fields().items()}


def _assert_follows(records, want, what):
    """Every recorded fields() row against the restatement, exactly."""
    for i, (rec, w) in enumerate(zip(records, want)):
        got = {k: (np.float32(float(rec[k])) if k == "scale" else int(rec[k])) for k in R.SCALER_FIELDS}
        assert got == w, f"{what}: step {i}: the kernel's {got}, the rule's {w}"


def _all_finite(torch, tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def test_backoff_stops_at_the_floor(torch_cuda):
    """200 consecutive steps with an injected inf, from the default 65536."""
    torch = torch_cuda
    opt, params, gbufs, _ = _adam(torch, init_scale=65536.0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for g in gbufs:
        g.copy_(torch.randn(g.shape, device="cuda", generator=gen) * 1e-2 * 65536.0)
    gbufs[0][3, 5] = float("inf")
    before = [t.clone() for t in params + opt.exp_avg + opt.exp_avg_sq]
    st, records, want = R.scaler_state(65536.0), [], []
    for _ in range(200):
        opt.step()
        records.append(_record(opt))
        st = R.scaler_update(st, False, DYNAMIC)
        want.append(st)
    _assert_follows(records, want, "backoff")
    assert int(records[-1]["skipped"]) == 200 and int(records[-1]["step"]) == 0 and float(records[-1]["scale"]) == 1.0
    for x, y in zip(before, params + opt.exp_avg + opt.exp_avg_sq):
        assert torch.equal(x, y)
    print(f"  200 skipped steps: scale {float(records[-1]['scale'])}, floor hits {int(records[-1]['floor_hits'])}")


START_SCALES = [("1", 1.0), ("2^-100", 2.0 ** -100), ("2^-126", 2.0 ** -126), ("2^-127", 2.0 ** -127), ("denorm_min", DENORM_MIN), ("0", 0.0),
                ("2^126", 2.0 ** 126), ("2^127", 2.0 ** 127)]


def _gradients(torch, kind, gen):
    """Unscaled gradients, fp32 on the host.  small: N(0, 1e-2).  sparse: 12 elements per tensor with 1 <= |g| < 1.5 — times 2^-126 they are
    still normal numbers, times 2^127 still finite — and zeros elsewhere: 36 elements, a norm below sqrt(36 x 2.25) = 9 < max_norm, so the
    clip stays inactive like the small set's (the cases ask what the scale does, and a clip coefficient times 1 / 2^127 would be a
    denormal factor).  zero: all zero."""
    out = []
    for s in SHAPES:
        if kind == "small":
            g = torch.randn(s, generator=gen) * 1e-2
        elif kind == "zero":
            g = torch.zeros(s)
        else:
            g = torch.zeros(s)
            n = g.numel()
            at = torch.randperm(n, generator=gen)[:12]
            g.view(-1)[at] = (1.0 + 0.5 * torch.rand(at.numel(), generator=gen)) * (torch.randint(0, 2, (at.numel(),), generator=gen) * 2.0 - 1.0)
        out.append(g.numpy().astype(np.float32))
    return out


@pytest.mark.parametrize("kind", ["small", "sparse", "zero"])
@pytest.mark.parametrize("name,s0", START_SCALES)
def test_one_clean_step_at_an_extreme_scale(torch_cuda, name, s0, kind):
    """The start scale in both state rows (what a loaded checkpoint leaves), one step on the finite gradients fl(g x s0), formed in fp32 as the
    loss kernel and the backward leave them."""
    torch = torch_cuda
    opt, params, gbufs, p0 = _adam(torch, init_scale=65536.0)
    _set_scale(torch, opt, s0)
    gs_unscaled = _gradients(torch, kind, torch.Generator().manual_seed(77))
    with np.errstate(under="ignore"):
        scaled = [g * F32(s0) for g in gs_unscaled]
    assert all(np.isfinite(x).all() for x in scaled)
    exact = s0 > 0 and all(np.array_equal(x.astype(np.float64) / s0, g.astype(np.float64)) for x, g in zip(scaled, gs_unscaled))
    for buf, x in zip(gbufs, scaled):
        buf.copy_(torch.from_numpy(x).cuda())
        assert torch.equal(_bits(torch, buf.cpu()), _bits(torch, torch.from_numpy(x)))     # denormals arrived as they are
    st0 = R.scaler_state(s0)
    assert float(opt.fields()["scale"]) == s0
    before = [t.clone() for t in params + opt.exp_avg + opt.exp_avg_sq]
    opt.step()
    torch.cuda.synchronize()
    after = params + opt.exp_avg + opt.exp_avg_sq
    steps = R.scaler_steps(st0, True)
    print(f"  s0={name} {kind}: g x s0 exact {exact}, the rule steps {steps}; fields {({k: float(v) for k, v in opt.fields().items()})}")
    assert _all_finite(torch, after), [i for i, t in enumerate(after) if not bool(torch.isfinite(t).all())]
    _assert_follows([_record(opt)], [R.scaler_update(st0, True, DYNAMIC)], f"s0={name} {kind}")
    if not steps:
        for x, y in zip(before, after):
            assert torch.equal(x, y)
    elif exact:
        tp, topt = _torch_adam(torch, p0, 1e-3)
        for q, g in zip(tp, gs_unscaled):
            q.grad = torch.from_numpy(g).double()
        assert float(torch.nn.utils.clip_grad_norm_(tp, 10.0)) < 10.0
        topt.step()
        worst = _assert_adam_close(torch, opt, params, tp, topt, f"s0={name} {kind}")
        print(f"    against torch's fp64 Adam on g: worst error {worst:.3g} of the tolerance")
    assert name not in ("1", "2^-100", "2^126", "2^127") or (exact and steps)
    assert name != "2^-126" or (steps and exact == (kind != "small"))


def test_growth_stops_below_inf(torch_cuda):
    """400 clean steps on all-zero gradients from 2^120: finite after every step."""
    torch = torch_cuda
    opt, params, gbufs, _ = _adam(torch, init_scale=2.0 ** 120)
    st, records, want = R.scaler_state(2.0 ** 120), [], []
    for _ in range(400):
        opt.step()
        records.append(_record(opt))
        st = R.scaler_update(st, True, DYNAMIC)
        want.append(st)
    scales = [float(r["scale"]) for r in records]
    assert np.isfinite(scales).all(), scales[:30]
    _assert_follows(records, want, "growth")
    assert max(scales) == 2.0 ** 127 and int(records[-1]["step"]) == 400 and int(records[-1]["skipped"]) == 0
    assert _all_finite(torch, params + opt.exp_avg + opt.exp_avg_sq)


def test_constant_scale_is_untouched_by_the_bounds(torch_cuda):
    """dynamic=False at scale 1: test_ppo_edges_gpu.test_adam_constant_scale's assertions on this file's tensors, and the rule with factors 1."""
    torch = torch_cuda
    opt, params, gbufs, p0 = _adam(torch, seed=21, init_scale=1.0, dynamic=False)
    tp, topt = _torch_adam(torch, [p.clone() for p in p0], 1e-3)
    gen = torch.Generator().manual_seed(22)
    read = lambda: {k: float(v) for k, v in opt.fields().items()}
    st, worst, clean = R.scaler_state(1.0), 0.0, 0
    for step in range(9):
        for buf, q in zip(gbufs, tp):
            g = torch.randn(buf.shape, generator=gen) * 1e-2
            buf.copy_(g.cuda())
            q.grad = g.double()
        bad = {2: float("inf"), 5: float("nan")}.get(step)
        if bad is not None:
            gbufs[1][7, 5] = bad
            before = [t.clone() for t in params + opt.exp_avg + opt.exp_avg_sq]
        else:
            torch.nn.utils.clip_grad_norm_(tp, 10.0)
            topt.step()
            clean += 1
        opt.step()
        s = read()
        st = R.scaler_update(st, bad is None, CONSTANT)
        _assert_follows([_record(opt)], [st], f"constant scale, step {step}")
        assert s["scale"] == 1.0 and s["step"] == clean and s["skipped"] == step + 1 - clean and s["floor_hits"] == 0, (step, s)
        if bad is not None:
            for x, y in zip(before, params + opt.exp_avg + opt.exp_avg_sq):
                assert torch.equal(x, y)
        else:
            worst = max(worst, _assert_adam_close(torch, opt, params, tp, topt, f"step {step}"))
    print(f"  constant scale: worst error {worst:.3g} of the tolerance")


# ======================================================================================================================================
# D. the pieces together
# ======================================================================================================================================
def _minibatch(torch, lr, loss, opt, obs, logstd, make_rows, stats):
    """PPOTrainer.minibatch_step's sequence on given objects; make_rows(mu, value) -> the batch dict around the forward's own mu."""
    mu, value = lr.forward(obs)
    b = make_rows(_np(mu).copy(), _np(value).reshape(-1).copy())
    d = lambda k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda()
    old_head = torch.zeros((obs.shape[0], mu.shape[1] + 1), device="cuda")
    old_head[:, :mu.shape[1]] = d("old_mu")
    d_head = loss(mu, value, d("actions"), old_head[:, :mu.shape[1]], d("old_sigma"), d("old_neglogp"), d("advantages"), d("old_values"),
                  d("returns"), logstd, opt.scale, stats)
    lr.backward(d_head)
    opt.step()
    lr.sync_weights()
    return d_head


def test_overflow_burst_then_healthy_minibatches(torch_cuda):
    """160 minibatches that overflow by construction (log ratio 8e3 under a negative advantage: d_head holds inf), then healthy ones
    (test_ppo_gpu._batch's rows around the network's own mu)."""
    torch = torch_cuda
    from isaacgym_amd import ppo
    from isaacgym_amd.policy import NativeMLPLearner
    from test_policy_mlp import _mlp
    m, num_obs, a = 64, 80, 7
    gen = torch.Generator().manual_seed(9)
    lr = NativeMLPLearner(_mlp(torch, num_obs, (256, 128), a, gen), _mlp(torch, num_obs, (256, 128), 1, gen), num_obs, "cuda:0", head_grad_extra=a)
    logstd = torch.full((a,), -2.0, device="cuda")
    cfg = ppo.PPOConfig()
    loss = ppo.LossGrad(a, m, "cuda", cfg, d_logstd=lr.grad_extra)
    opt = ppo.DeviceAdam(lr.parameters() + [logstd], lr.gradients() + [lr.grad_extra], 1e-3, max_norm=cfg.grad_norm, truncate=True, init_scale=512.0,
                         growth_interval=3)
    obs = torch.randn(m, num_obs, generator=gen).cuda()
    stats = torch.zeros(8, device="cuda")
    rng = np.random.default_rng(9)
    ls = _np(logstd)

    def unhealthy(mu, value):
        return R.rows_around(rng, mu, ls, np.full(m, 8e3), -(0.05 + np.abs(rng.standard_normal(m))), value,
                             value - rng.choice([-50.0, -5.0, 5.0, 50.0], m) * rng.uniform(0.6, 1.0, m), rng.uniform(-1e3, 1e3, m))

    def healthy(mu, value):
        # (value is the network's: old_values are placed around it instead of the other way round)
        return R.rows_around(rng, mu, ls, rng.choice(R.HEALTHY_C, m), rng.standard_normal(m), value, value - rng.choice([-0.5, -0.1, 0.1, 0.5], m),
                             rng.standard_normal(m))

    everything = lambda: lr.parameters() + [logstd] + opt.exp_avg + opt.exp_avg_sq
    before = [t.clone() for t in everything()]
    st, records, want = R.scaler_state(512.0), [], []
    for k in range(160):
        d_head = _minibatch(torch, lr, loss, opt, obs, logstd, unhealthy, stats)
        if k == 0:
            assert bool(torch.isinf(d_head[:, :a]).all(1).all())   # every row overflows
        records.append(_record(opt))
        st = R.scaler_update(st, False, DYNAMIC)
        want.append(st)
    for x, y in zip(before, everything()):
        assert torch.equal(x, y)
    _assert_follows(records, want, "overflow burst")
    assert float(records[-1]["scale"]) == 1.0 and int(records[-1]["skipped"]) == 160
    scales = []
    for k in range(4):
        _minibatch(torch, lr, loss, opt, obs, logstd, healthy, stats)
        f = {k_: float(v) for k_, v in opt.fields().items()}
        print(f"  healthy minibatch {k}: {f}; loss {float(stats[0]):.6g}")
        assert _all_finite(torch, everything()), f"healthy minibatch {k}"
        assert np.isfinite(_np(stats)).all()
        assert f["step"] == k + 1 and f["skipped"] == 160
        scales.append(f["scale"])
    assert scales == [1.0, 1.0, 2.0, 2.0]
    assert all(not torch.equal(x, y) for x, y in zip(before[:len(lr.parameters()) + 1], lr.parameters() + [logstd]))


def test_trainer_resumes_from_a_denormal_scale(torch_cuda):
    """A trainer whose scaler rows hold the smallest denormal (the checkpoint of a run whose scale had no floor): two epochs."""
    torch = torch_cuda
    from test_ppo_critic_input_gpu import TT, trainer
    tr = trainer(TT)
    _set_scale(torch, tr.opt, DENORM_MIN)
    assert float(tr.opt.scale) == DENORM_MIN
    for epoch in range(2):
        res = {k: float(v) for k, v in tr.train_epoch().items()}
        print(f"  epoch {epoch}: {res}")
        assert all(np.isfinite(v) for v in res.values()), res
        assert all(bool(torch.isfinite(p).all()) for p in tr.learner.parameters() + [tr.logstd] + tr.opt.exp_avg + tr.opt.exp_avg_sq)
    f = {k: float(v) for k, v in tr.opt.fields().items()}
    assert f["scale"] >= 1.0 and f["floor_hits"] >= 1 and f["step"] > 0
