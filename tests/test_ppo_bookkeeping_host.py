"""PPOTrainer's bookkeeping on the CPU (no GPU): `_episodes` (the printed return / length) against a per-row loop over carried horizons,
and `prepare()` (old_neglogp, advantage and value normalisation: everything the loss kernel reads) against a plain fp64 restatement
(tests/ppo_reference.py), which is itself checked here against an independent formulation (torch.distributions, torch.var, the law of total
variance).  The trainer's methods are called unbound on stubs that carry only the attributes they read; the value statistics' device kernel
is replaced by a torch double of the same interface (the kernel itself: test_policy_backward.py, test_ppo_edges_gpu.py)."""
import math
import types

import numpy as np
import pytest
import torch

import ppo_reference as R
from isaacgym_amd import ppo

U32 = R.U32


# ---- _episodes -----------------------------------------------------------------------------------------------------------------------
def _episode_stub(H, n):
    return types.SimpleNamespace(device=torch.device("cpu"), cfg=types.SimpleNamespace(horizon_length=H),
                                 col=types.SimpleNamespace(rewards=torch.zeros(H, n), dones=torch.zeros(H, n, dtype=torch.int64)),
                                 ep_ret=torch.zeros(n), ep_len=torch.zeros(n))


def _dones(kind, rng, H, n, horizon):
    d = np.zeros((H, n), dtype=np.int64)
    if kind == "none":
        pass
    elif kind == "every":
        d[:] = 1
    elif kind == "first":
        d[0] = 1
    elif kind == "last":
        d[H - 1] = 1
    elif kind == "back_to_back":                 # runs of two and three consecutive dones, at the horizon's ends and inside, rows staggered
        for i in range(n):
            s = (i + 3 * horizon) % H
            d[s, i] = d[(s + 1) % H, i] = 1
            if i % 3 == 0:
                d[(s + 2) % H, i] = 1
    else:
        d[:] = rng.random((H, n)) < float(kind)
    return d


CASES = [("none", 8, 5), ("every", 8, 5), ("first", 8, 5), ("last", 8, 5), ("back_to_back", 8, 11), ("0.3", 1, 40), ("0.3", 8, 1), ("0.05", 32, 64),
         ("0.05", 32, 1000)]


@pytest.mark.parametrize("kind,H,n", CASES)
def test_episodes_equal_a_per_row_loop_on_integer_rewards(kind, H, n):
    """Small-integer rewards: every fp32 sum is exact, so sums, lengths, count and the carried state are equal, over four carried horizons."""
    rng = np.random.default_rng(H * 1000 + n)
    stub = _episode_stub(H, n)
    ep_ret, ep_len = np.zeros(n), np.zeros(n)
    finished = 0
    for horizon in range(4):
        rew, done = rng.integers(-3, 5, (H, n)).astype(np.float32), _dones(kind, rng, H, n, horizon)
        if horizon == 2:
            done = done * rng.choice([1, 2, 2 ** 32], (H, n))            # any non-zero value is a done
        stub.col.rewards.copy_(torch.from_numpy(rew))
        stub.col.dones.copy_(torch.from_numpy(done))
        out = ppo.PPOTrainer._episodes(stub)
        want = R.episodes_loop(rew, done, ep_ret, ep_len)
        ep_ret, ep_len = want["ep_ret"], want["ep_len"]
        assert out.dtype == torch.float32 and out.tolist() == [want["sum_ret"], want["sum_len"], float(want["count"])], (horizon, out, want)
        assert np.array_equal(stub.ep_ret.numpy().astype(np.float64), ep_ret), horizon
        assert np.array_equal(stub.ep_len.numpy().astype(np.float64), ep_len), horizon
        finished += want["count"]
    assert (finished == 0) == (kind == "none")
    if kind == "none":
        assert ep_len.tolist() == [4.0 * H] * n


def test_episodes_real_rewards_within_the_running_sums_rounding():
    """Rewards of the tasks' magnitude (a few units per step, bonuses of tens).  The tolerance is ppo_reference.episodes_loop's: 2 H 2^-24
    max_t |cumsum| per finished episode and horizon, from the fp64 loop."""
    H, n = 32, 512
    rng = np.random.default_rng(11)
    stub = _episode_stub(H, n)
    ep_ret, ep_len, ep_err = np.zeros(n), np.zeros(n), np.zeros(n)
    worst = 0.0
    for horizon in range(5):
        rew = (rng.normal(2.0, 3.0, (H, n)) + 40.0 * (rng.random((H, n)) < 0.02)).astype(np.float32)
        done = (rng.random((H, n)) < 0.03).astype(np.int64)
        stub.col.rewards.copy_(torch.from_numpy(rew))
        stub.col.dones.copy_(torch.from_numpy(done))
        out = ppo.PPOTrainer._episodes(stub).double().numpy()
        want = R.episodes_loop(rew, done, ep_ret, ep_len, ep_err)
        ep_ret, ep_len, ep_err = want["ep_ret"], want["ep_len"], want["ep_err"]
        assert want["count"] > 0
        bound = want["bound"] + U32 * abs(want["sum_ret"])                 # + the fp32 result's own rounding
        err = abs(out[0] - want["sum_ret"])
        worst = max(worst, err / bound)
        assert err <= bound, (horizon, out[0], want["sum_ret"], bound)
        assert out[1] == want["sum_len"] and out[2] == want["count"]
        assert np.array_equal(stub.ep_len.numpy().astype(np.float64), ep_len)
        assert (np.abs(stub.ep_ret.numpy().astype(np.float64) - ep_ret) <= ep_err + U32 * np.abs(ep_ret)).all()
    print(f"episode returns: worst error / bound {worst:.3g}")


# ---- the restatement of prepare() against an independent formulation -----------------------------------------------------------------
def _rollout(rng, H, n, A, outliers=True):
    """A horizon's buffers of the collector's shapes, values and returns far from zero mean, a few beyond 5 sigma of the statistics to come."""
    sigma = np.exp(rng.uniform(-2.2, -1.8, A)).astype(np.float32)
    head = rng.uniform(-1.2, 1.2, (H + 1, n, A + 1)).astype(np.float32)
    head[:, :, A] = rng.normal(3.0, 0.7, (H + 1, n))
    actions = np.clip(head[:H, :, :A] + sigma * rng.standard_normal((H, n, A)), -1, 1).astype(np.float32)
    returns = (head[:H, :, A] + rng.normal(0.4, 0.5, (H, n))).astype(np.float32)
    if outliers:
        head[1, 0, A], head[2, n - 1, A] = 40.0, -30.0
        returns[0, 0], returns[H - 1, n - 1] = 55.0, -45.0
    advantages = (returns - head[:H, :, A]).astype(np.float32)
    return dict(sigma=sigma, head=head, actions=actions, returns=returns, advantages=advantages)


class TorchRMS:
    """The interface of policy.RunningMeanStd that prepare() uses, in torch fp64: batch moments by torch.mean / torch.var, merged as two
    groups by the law of total variance (algebraically rl_games' parallel-moments rule, written differently from ppo_reference.rms_merge)."""

    def __init__(self, eps=1e-5):
        self.m, self.v, self.c, self.eps = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64), 1.0, eps
        self.refresh()

    def refresh(self):
        self.mean, self.inv_std = self.m.float().view(1), torch.rsqrt(self.v + self.eps).float().view(1)

    def update(self, x):
        x = x.double().view(-1)
        k, bm, bv = x.numel(), x.mean(), x.var()
        tot = self.c + k
        m = (self.c * self.m + k * bm) / tot
        self.v = (self.c * (self.v + (self.m - m) ** 2) + k * (bv + (bm - m) ** 2)) / tot
        self.m, self.c = m, tot
        self.refresh()

    def state(self):
        return float(self.m), float(self.v), float(self.c)


def test_prepare_reference_matches_an_independent_formulation():
    rng = np.random.default_rng(2)
    H, n, A = 8, 40, 7
    rms = TorchRMS()
    for epoch in range(3):
        b = _rollout(rng, H, n, A)
        total = H * n
        act, mu = b["actions"].reshape(total, A), b["head"][:H].reshape(total, A + 1)[:, :A]
        v, r, adv = b["head"][:H, :, A].reshape(total), b["returns"].reshape(total), b["advantages"].reshape(total)
        before = rms.state()
        got = R.prepare_reference(act, mu, b["sigma"], v, r, adv, rms_state=before)
        t = lambda x: torch.from_numpy(np.asarray(x)).double()
        nlp = -torch.distributions.Normal(t(mu), t(b["sigma"])).log_prob(t(act)).sum(-1)
        np.testing.assert_allclose(got["old_nlp"], nlp.numpy(), rtol=1e-12)
        a = t(adv)
        np.testing.assert_allclose(got["adv"], ((a - a.mean()) / (torch.var(a, unbiased=True).sqrt() + 1e-8)).numpy(), rtol=1e-11, atol=1e-13)
        norm = lambda x: ((t(x) - rms.m) / torch.sqrt(rms.v + 1e-5)).clamp(-5.0, 5.0).numpy()
        rms.update(t(v))
        np.testing.assert_allclose(got["old_v"], norm(v), rtol=1e-11, atol=1e-13)
        rms.update(t(r))
        np.testing.assert_allclose(got["ret"], norm(r), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(got["rms_state"], rms.state(), rtol=1e-12)
        assert (np.abs(got["old_v"]) == 5.0).sum() >= 2 and (np.abs(got["ret"]) == 5.0).sum() >= 2        # the clamp is exercised
        off = R.prepare_reference(act, mu, b["sigma"], v, r, adv, rms_state=None, normalize_advantage=False)
        assert np.array_equal(off["adv"], adv.astype(np.float64)) and np.array_equal(off["old_v"], v.astype(np.float64))
        assert np.array_equal(off["ret"], r.astype(np.float64)) and off["rms_state"] is None


def test_gae_loop_and_denorm_match_torch_fp64():
    rng = np.random.default_rng(4)
    H, n = 6, 9
    rew, val, done = rng.normal(0, 50, (H, n)), rng.normal(3, 1, (H + 1, n)), (rng.random((H, n)) < 0.3).astype(np.int64)
    got = R.gae_loop(rew, val, done, 0.99, 0.95, 0.01)
    r, v, nd = torch.from_numpy(rew), torch.from_numpy(val), 1.0 - torch.from_numpy(done).double()
    run, want = torch.zeros(n, dtype=torch.float64), torch.zeros(H, n, dtype=torch.float64)
    for t in reversed(range(H)):
        run = 0.01 * r[t] + 0.99 * v[t + 1] * nd[t] - v[t] + 0.99 * 0.95 * nd[t] * run
        want[t] = run
    np.testing.assert_allclose(got["adv"], want.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(got["ret"], (want + v[:H]).numpy(), rtol=1e-13, atol=1e-15)
    x = np.array([-7.0, -5.0, 0.3, 5.0, 9.0])
    np.testing.assert_allclose(R.rms_denorm(x, (2.0, 9.0, 10.0), eps=0.0), [-13.0, -13.0, 2.9, 17.0, 17.0], rtol=1e-15)
    np.testing.assert_allclose(R.rms_norm(R.rms_denorm(x, (2.0, 9.0, 10.0)), (2.0, 9.0, 10.0)), np.clip(x, -5, 5), rtol=1e-14)


# ---- prepare() itself, on a CPU stub --------------------------------------------------------------------------------------------------
def _prepare_stub(b, H, n, A, rms, normalize_advantage):
    total = H * n
    col = types.SimpleNamespace(actions=torch.from_numpy(b["actions"]), head=torch.from_numpy(b["head"]), sigma=torch.from_numpy(b["sigma"]),
                                returns=torch.from_numpy(b["returns"]), advantages=torch.from_numpy(b["advantages"]))
    col.values = col.head[:, :, A]
    z = lambda: torch.zeros(total)
    return types.SimpleNamespace(col=col, cfg=types.SimpleNamespace(horizon_length=H, normalize_advantage=normalize_advantage), rows=n, num_actions=A,
                                 old_nlp=z(), adv=z(), old_v=z(), ret=z(), value_rms=rms)


@pytest.mark.parametrize("normalize_value,normalize_advantage", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("A", [1, 7, 27])
def test_prepare_matches_the_fp64_restatement(A, normalize_value, normalize_advantage):
    """Three epochs on one set of value statistics (so the second and third start from a state that is not the initial one); values and
    returns include entries beyond 5 sigma, so a missing clamp shows."""
    rng = np.random.default_rng(A)
    H, n = 8, 24
    total = H * n
    rms = TorchRMS() if normalize_value else None
    worst = {}
    for epoch in range(3):
        b = _rollout(rng, H, n, A)
        stub = _prepare_stub(b, H, n, A, rms, normalize_advantage)
        before = rms.state() if rms is not None else None
        ppo.PPOTrainer.prepare(stub)
        v, r, adv = b["head"][:H, :, A].reshape(total), b["returns"].reshape(total), b["advantages"].reshape(total)
        ref = R.prepare_reference(b["actions"].reshape(total, A), b["head"][:H].reshape(total, A + 1)[:, :A], b["sigma"], v, r, adv, rms_state=before,
                                  normalize_advantage=normalize_advantage)
        if rms is not None:
            np.testing.assert_allclose(rms.state(), ref["rms_state"], rtol=1e-12)
            mid = R.rms_merge(before, v)
            bounds = dict(old_nlp=R.nlp_bound(ref, A), old_v=R.norm_bound(v, mid), ret=R.norm_bound(r, ref["rms_state"]))
            assert (np.abs(ref["old_v"]) == 5.0).any() and (np.abs(ref["ret"]) == 5.0).any()
        else:
            bounds = dict(old_nlp=R.nlp_bound(ref, A), old_v=0.0 * v, ret=0.0 * r)               # plain copies: equal
        bounds["adv"] = R.adv_bound(adv, total) if normalize_advantage else 0.0 * adv
        for k, bound in bounds.items():
            err = np.abs(getattr(stub, k).numpy().astype(np.float64) - ref[k])
            bound = bound + U32 * np.abs(ref[k]) * (np.asarray(bound) > 0)                     # the fp32 result's own rounding
            assert (err <= bound).all(), (k, epoch, float((err - bound).max()))
            ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
            worst[k] = max(worst.get(k, 0.0), ratio)
    print("prepare() on the CPU, worst error / bound:", {k: round(v, 3) for k, v in worst.items()})
