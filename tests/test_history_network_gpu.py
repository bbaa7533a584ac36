"""The native network at the first-layer widths an observation and action history gives it (include/ppenv_history.h): K = 3 * 80 + 2 * 7 =
254, padded to 256, and K = 3 * 313 + 2 * 27 = 993, padded to 1024 — forward and backward of the actor / critic pair, input statistics
included, against PyTorch autograd in fp32 on the same weights, under the tolerances tests/test_policy_backward.py uses for the narrow
network (restated below, not widened).  128 rows.  Need a real MI355X."""
import pytest

from test_policy_mlp import _mlp

pytestmark = pytest.mark.gpu

RTOL, ATOL_OF_SCALE, MEAN_OF_SCALE = 1e-2, 1e-2, 2e-3      # test_native_backward_matches_fp32_autograd's: |err| <= RTOL |want| + ATOL_OF_SCALE max|want|, mean |err| < MEAN_OF_SCALE max|want|
UNITS = (2048, 1536, 1024, 1024, 512, 512)


def close(name, got, want, mean=True):
    """mean: the gradients' second bound; the forward outputs are held to the element bound alone, as tests/test_policy_mlp.py holds them."""
    scale = float(want.abs().max())
    err = (got - want).abs()
    print(f"{name}: max err {float(err.max()):.3g} mean err {float(err.mean()):.3g} scale {scale:.3g}")
    assert bool((err <= RTOL * want.abs() + ATOL_OF_SCALE * scale).all()), (name, float(err.max()), scale)
    assert not mean or float(err.mean()) < MEAN_OF_SCALE * scale, (name, float(err.mean()), scale)


@pytest.mark.parametrize("n, a, ho, ha, padded", [(80, 7, 2, 2, 256), (313, 27, 2, 2, 1024)], ids=["K254", "K993"])
def test_forward_and_backward_at_the_wide_first_layer_match_fp32_autograd(n, a, ho, ha, padded):
    import torch
    from isaacgym_amd import history
    from isaacgym_amd.policy import NativeMLPLearner, RunningMeanStd
    m, k = 128, history.width(n, a, ho, ha)
    assert k == (ho + 1) * n + ha * a and (k + 63) // 64 * 64 == padded
    gen = torch.Generator().manual_seed(k)
    actor, critic = _mlp(torch, k, UNITS, a, gen), _mlp(torch, k, UNITS, 1, gen)
    wide = torch.randn(m, k, generator=gen) * 2.0 + 0.3
    wide[:, (ho + 1) * n:].clamp_(-1.0, 1.0)                     # the action slots hold clamped actions
    learner = NativeMLPLearner(actor, critic, k, "cuda:0")
    assert learner.net.w[0].shape[-1] == padded
    rms = RunningMeanStd(k, "cuda:0")
    learner.attach_running_mean_std(rms)
    mu, value = (t.clone() for t in learner.forward(wide.cuda(), update_stats=True))
    d_head = torch.randn(m, a + 1, generator=gen)
    d_head[:, a] *= 3.0
    grads = [g.clone() for g in learner.backward(d_head.cuda())]
    torch.cuda.synchronize()
    mean, inv_std = rms.mean.cpu(), rms.inv_std.cpu()
    x = torch.clamp((wide - mean) * inv_std, -5.0, 5.0)
    params = []

    def run(layers):
        h = x
        for i, (w, b) in enumerate(layers):
            w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            params.append((w, b))
            h = h @ w.t() + b
            if i + 1 < len(layers):
                h = torch.nn.functional.elu(h)
        return h
    out = torch.cat([run(actor), run(critic)], dim=1)
    close("mu", mu.cpu(), out[:, :a].detach(), mean=False)
    close("value", value.cpu(), out[:, a:].detach(), mean=False)
    out.backward(d_head)
    nl = len(UNITS)
    a_p, c_p = params[:nl + 1], params[nl + 1:]
    want = ([torch.stack([a_p[i][0].grad, c_p[i][0].grad]) for i in range(nl)] + [torch.stack([a_p[i][1].grad, c_p[i][1].grad]) for i in range(nl)] +
            [a_p[nl][0].grad, a_p[nl][1].grad, c_p[nl][0].grad, c_p[nl][1].grad])
    names = [f"w{i}" for i in range(nl)] + [f"b{i}" for i in range(nl)] + ["mu_w", "mu_b", "value_w", "value_b"]
    assert len(grads) == len(want) == len(learner.parameters())
    for name, g, w in zip(names, grads, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        close(name, g.cpu(), w)
    assert grads[0].shape[-1] == k                              # the first layer's gradient is K wide: the padding is not a parameter
