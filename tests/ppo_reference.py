"""Plain fp64 restatements (numpy, loops where a loop is the plainest form) of what PPOTrainer does between the rollout and the loss kernel:
the episode bookkeeping, GAE, the value de-normalisation and prepare().  Written from the rl_games formulas the trainer's docstrings name, not
from the torch code; tests/test_ppo_bookkeeping_host.py checks them against independent formulations on the CPU, and the GPU tests use them
as the reference.  At the end: the loss scale's rule in numpy float32 and the rows of a policy that has run away (tests/test_ppo_runaway_*.py)."""
import math

import numpy as np

U32 = 2.0 ** -24                      # unit roundoff of fp32
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def episodes_loop(rewards, dones, ep_ret, ep_len, ep_err=None):
    """One horizon, one row at a time: rewards / dones [H, n], the running episode's (return, length) per row [n].
    -> dict(sum_ret, sum_len, count, ep_ret, ep_len (carried on), bound: the fp32 bound of `sum_ret`, ep_err [n]: that of the carried ep_ret).
    The bound: the trainer forms an episode's sum as a difference of an fp32 running sum over the horizon, each end of which is off by at
    most H roundings of the largest running sum: 2 H 2^-24 max_t |cumsum| per episode and horizon, summed over the finished episodes; an
    episode carried in from earlier horizons (ep_err: their bounds) brings theirs along."""
    r, d = np.asarray(rewards, dtype=np.float64), np.asarray(dones) != 0
    H, n = r.shape
    ret, length = np.array(ep_ret, dtype=np.float64), np.array(ep_len, dtype=np.float64)
    err = np.zeros(n) if ep_err is None else np.array(ep_err, dtype=np.float64)
    sum_ret = sum_len = bound = 0.0
    count = 0
    for i in range(n):
        cs, peak = 0.0, abs(ret[i])
        for t in range(H):
            cs += r[t, i]
            ret[i] += r[t, i]
            peak = max(peak, abs(cs), abs(ret[i]))
        here = 2.0 * H * U32 * peak
        ret[i] = ep_ret[i]
        for t in range(H):
            ret[i] += r[t, i]
            length[i] += 1.0
            if d[t, i]:
                sum_ret += ret[i]
                sum_len += length[i]
                count += 1
                bound += here + err[i]
                ret[i], length[i], err[i] = 0.0, 0.0, 0.0
        err[i] += here
    return dict(sum_ret=sum_ret, sum_len=sum_len, count=count, ep_ret=ret, ep_len=length, bound=bound, ep_err=err)


def gae_loop(rewards, values, dones, gamma, tau, reward_scale):
    """rl_games discount_values: rewards / dones [H, n], values [H + 1, n] -> dict(adv, ret [H, n], bound [H, n]: the fp32 bound of both).
    The bound follows the recurrence: delta is three products and two sums of terms |s r|, gamma |v'|, |v| (5 roundings of the largest partial
    sum, itself at most their sum), the running advantage one product chain and one sum more (3), the return one sum (1); the error of the
    next step's advantage comes along times gamma tau."""
    r, v, nd = np.asarray(rewards, dtype=np.float64), np.asarray(values, dtype=np.float64), (np.asarray(dones) == 0).astype(np.float64)
    H, n = r.shape
    adv, bound = np.zeros((H, n)), np.zeros((H, n))
    run, err = np.zeros(n), np.zeros(n)
    for t in range(H - 1, -1, -1):
        terms = np.abs(reward_scale * r[t]) + gamma * np.abs(v[t + 1]) * nd[t] + np.abs(v[t])
        run = reward_scale * r[t] + gamma * v[t + 1] * nd[t] - v[t] + gamma * tau * nd[t] * run
        err = U32 * (5.0 * terms + 3.0 * (np.abs(run) + terms)) + gamma * tau * nd[t] * err
        adv[t] = run
        bound[t] = err + U32 * (np.abs(run) + np.abs(v[t]))
    return dict(adv=adv, ret=adv + v[:H], bound=bound)


def rms_merge(state, x):
    """rl_games RunningMeanStd._update_mean_var_count_from_moments on one batch x [m] (or [m, k]): state = (mean, var, count), the batch's
    mean and UNBIASED variance."""
    mean, var, count = state
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[0]
    bmean = x.sum(0) / m
    bvar = ((x - bmean) ** 2).sum(0) / (m - 1) if m > 1 else np.zeros_like(bmean)
    delta, tot = bmean - mean, count + m
    m2 = var * count + bvar * m + delta * delta * count * m / tot
    return mean + delta * m / tot, m2 / tot, tot


def rms_norm(x, state, eps=1e-5):
    mean, var, _ = state
    return np.clip((np.asarray(x, dtype=np.float64) - mean) / np.sqrt(var + eps), -5.0, 5.0)


def rms_denorm(x, state, eps=1e-5):
    """rl_games RunningMeanStd(unnorm=True): clamp(+-5), then x sqrt(var + eps) + mean."""
    mean, var, _ = state
    return np.clip(np.asarray(x, dtype=np.float64), -5.0, 5.0) * np.sqrt(var + eps) + mean


def prepare_reference(actions, mu, sigma, values, returns, advantages, rms_state=None, normalize_advantage=True):
    """What the loss kernel is fed: actions / mu [M, A], sigma [A], values / returns / advantages [M]; rms_state: the value statistics
    (mean, var, count) as scalars before the epoch, or None without normalize_value.
    -> dict(old_nlp, adv, old_v, ret [M], rms_state (after), nlp_terms [M]: sum of the absolute terms of old_nlp, for its fp32 bound)."""
    f = lambda t: np.asarray(t, dtype=np.float64)
    act, mu, sg, v, r, adv = f(actions), f(mu), f(sigma), f(values).reshape(-1), f(returns).reshape(-1), f(advantages).reshape(-1)
    M, A = act.shape
    old_nlp, terms = np.zeros(M), np.zeros(M)
    logs = np.log(sg)
    for j in range(A):
        z = (act[:, j] - mu[:, j]) / sg[j]
        old_nlp += 0.5 * z * z + HALF_LOG_2PI + logs[j]
        terms += 0.5 * z * z + HALF_LOG_2PI + abs(logs[j])
    if normalize_advantage:
        centred = adv - adv.sum() / M
        std = math.sqrt((centred ** 2).sum() / (M - 1))           # torch.std: unbiased
        adv = centred / (std + 1e-8)
    if rms_state is None:
        old_v, ret = v, r
    else:                                                          # values first, then returns, each normalised right after its update
        rms_state = rms_merge(rms_state, v)
        old_v = rms_norm(v, rms_state)
        rms_state = rms_merge(rms_state, r)
        ret = rms_norm(r, rms_state)
    return dict(old_nlp=old_nlp, adv=adv, old_v=old_v, ret=ret, rms_state=rms_state, nlp_terms=terms)


# ---- fp32 bounds of prepare()'s outputs, from the fp64 data ---------------------------------------------------------------------------
def adv_bound(adv_raw, M):
    """fp32 bound per element of (adv - mean) / (std + 1e-8), from the fp64 data.  A reduction over M elements is taken as a tree / cascade
    sum whose longest chain is D = 2 ceil(log2 M) additions (torch's CPU and GPU reductions both are; a serial sum would be M): the mean is off
    by D u mean|adv|, the std relatively by D u; the subtraction, the + 1e-8 and the division round once each."""
    a = np.asarray(adv_raw, dtype=np.float64)
    D = 2.0 * math.ceil(math.log2(M))
    mean = a.mean()
    std = a.std(ddof=1)
    return U32 * ((np.abs(a - mean) + D * np.abs(a).mean()) / std + np.abs(a - mean) / std * (D + 3.0))


def norm_bound(x, state, eps=1e-5):
    """fp32 bound per element of clamp((x - mean32) * inv_std32): the fp32 image of the mean is off by u |mean|, that of 1 / sqrt(var + eps) by 4 u
    relatively (the cast, the sum, the root, the division), the subtraction and the product round once each; the clamp does not widen it."""
    mean, var, _ = state
    sd = math.sqrt(var + eps)
    return U32 * (abs(mean) / sd + 6.0 * np.abs((np.asarray(x, dtype=np.float64) - mean) / sd))


def nlp_bound(ref, A):
    """(A + 4) u sum |terms|: each z^2 carries the roundings of the subtraction, the division (twice in the square) and the square (5 u), the
    sum over the actions A - 1 more; the logs one each, their sum and the two additions the same count again."""
    return (A + 4.0) * U32 * ref["nlp_terms"]


# ---- the loss scale's rule, and rows where the policy has run away (tests/test_ppo_runaway_*.py) -----------------------------------------
F32 = np.float32
SCALE_FLOOR = F32(1.0)                # PPENV_PPO_SCALE_FLOOR (include/ppenv_ppo.h)
MIN_NORMAL = F32(2.0 ** -126)         # the smallest scale whose reciprocal is finite whether or not denormals are flushed
SCALER_FIELDS = ("scale", "growth_tracker", "step", "skipped", "floor_hits")
DYNAMIC = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
CONSTANT = dict(growth_factor=1.0, backoff_factor=1.0, growth_interval=3)


def scaler_steps(state, finite):
    """Does ppenv_ppo_adam_step take the step?  `finite`: the square sum of the (scaled) gradients is finite.  A scale that is not a normal
    positive fp32 number (0, a denormal, negative, NaN) cannot be divided out with a finite reciprocal: the step is skipped."""
    return bool(finite) and bool(F32(state["scale"]) >= MIN_NORMAL)


def scaler_update(state, finite, hp):
    """include/ppenv_ppo.h's scaler rule in numpy float32: state = dict over SCALER_FIELDS (scale: fp32), hp = dict(growth_factor,
    backoff_factor, growth_interval) -> the next state.  torch's GradScaler.update, with two bounds torch does not have: a dynamic scale
    (backoff_factor < 1) never leaves an update below SCALE_FLOOR — a state found below it is lifted — and growth is withheld where
    scale x growth_factor is not finite."""
    scale = F32(state["scale"])
    nx = dict(state)
    with np.errstate(all="ignore"):
        if not scaler_steps(state, finite):
            nx["scale"] = scale * F32(hp["backoff_factor"])
            nx["growth_tracker"] = 0
            nx["skipped"] = state["skipped"] + 1
        else:
            nx["step"] = state["step"] + 1
            nx["growth_tracker"] = state["growth_tracker"] + 1
            if nx["growth_tracker"] >= hp["growth_interval"]:
                grown = scale * F32(hp["growth_factor"])
                if np.isfinite(grown):
                    nx["scale"] = grown
                nx["growth_tracker"] = 0
        if hp["backoff_factor"] < 1.0 and not nx["scale"] >= SCALE_FLOOR:       # `not >=`: a NaN scale is lifted too
            nx["scale"] = SCALE_FLOOR
            nx["floor_hits"] = state["floor_hits"] + 1
    nx["scale"] = F32(nx["scale"])
    return nx


def scaler_state(scale, growth_tracker=0, step=0, skipped=0, floor_hits=0):
    return dict(scale=F32(scale), growth_tracker=growth_tracker, step=step, skipped=skipped, floor_hits=floor_hits)


RUNAWAY_C = (-8e3, -100.0, -80.0, -0.6, 0.0, 0.6, 80.0, 100.0, 8e3)      # log ratios: 0, fp32-denormal, normal, inf in fp32 only, inf in fp64
HEALTHY_C = (-0.6, -0.05, 0.0, 0.05, 0.6)                                 # test_ppo_gpu._batch's


def neglogp64(actions, mu, logstd):
    f = lambda x: np.asarray(x, dtype=np.float64)
    ls = f(logstd)
    z = (f(actions) - f(mu)) / np.exp(ls)
    return 0.5 * (z * z).sum(1) + HALF_LOG_2PI * z.shape[1] + ls.sum()


def rows_around(rng, mu, logstd, c, advantages, value, old_values, returns):
    """test_ppo_gpu._batch's rows around a GIVEN mu [m, a] (drawn, or a network's output): the actions are the clamped samples, old_mu and
    old_sigma lie near mu and sigma, and old_neglogp = nlp + c + U(+-0.02) with nlp formed in fp64 from the fp32 images, so that the log
    ratio the kernel sees is c up to old_neglogp's own fp32 rounding.  -> the fp32 batch dict of ppo.loss_grad_reference's arguments."""
    m, a = mu.shape
    mu, logstd = np.asarray(mu, dtype=F32), np.asarray(logstd, dtype=F32)
    sg = np.exp(logstd.astype(np.float64))
    actions = np.clip(mu + sg * rng.standard_normal((m, a)), -1, 1).astype(F32)
    old_nlp = neglogp64(actions, mu, logstd) + c + rng.uniform(-0.02, 0.02, m)
    b = dict(mu=mu, value=value, actions=actions, old_neglogp=old_nlp, old_mu=mu + 0.1 * rng.standard_normal((m, a)),
             old_sigma=sg * rng.uniform(0.9, 1.1, a), advantages=advantages, old_values=old_values, returns=returns, logstd=logstd)
    return {k: np.asarray(v, dtype=F32) for k, v in b.items()}


def runaway_batch(rng, m, a):
    """Rows of the regime DESIGN §6 records for seed 43: mu in +-20, log ratios from RUNAWAY_C, advantages of both signs with |adv| >= 0.05,
    value - old_values in +-[0.06, 0.1], [0.3, 0.5], [3, 5], [30, 50] (inside the value clip and far outside), returns in +-1e3.  The last
    m // 8 rows have adv == 0 and a log ratio within +-0.6 (an exact zero never meets an infinite ratio: 0 x inf is where numpy's maximum
    and fmaxf part, and the gradient is 0 either way)."""
    n0 = m // 8
    logstd = rng.uniform(-2.2, -1.5, a)
    mu = rng.uniform(-20.0, 20.0, (m, a))
    c = rng.choice(RUNAWAY_C, m)
    c[m - n0:] = rng.choice([-0.6, 0.0, 0.6], n0)
    adv = rng.choice([-1.0, 1.0], m) * (0.05 + np.abs(rng.standard_normal(m)))
    adv[m - n0:] = 0.0
    old_v = rng.standard_normal(m)
    value = old_v + rng.choice([-50.0, -5.0, -0.5, -0.1, 0.1, 0.5, 5.0, 50.0], m) * rng.uniform(0.6, 1.0, m)
    return rows_around(rng, mu, logstd, c, adv, value, old_v, rng.uniform(-1e3, 1e3, m))


def loss_grad_reference_f32_ratio(b, **kw):
    """ppo.loss_grad_reference with ONE change: the ratio is rounded to fp32 before it is used, the precision the kernel's header documents
    ("the ratio is formed in fp64; everything written is fp32").  The reference forms ratio = exp(old_neglogp - nlp) itself, so the rounding
    goes in through its argument: old_neglogp' = nlp + log(fp32(ratio)) in fp64 (-inf for a ratio of 0, +inf for an infinite one), which
    the reference's own exp turns back into fp32(ratio) to 1e-11 relatively."""
    from isaacgym_amd import ppo
    with np.errstate(all="ignore"):
        nlp = neglogp64(b["actions"], b["mu"], b["logstd"])
        ratio = np.exp(b["old_neglogp"].astype(np.float64) - nlp).astype(F32).astype(np.float64)
        return ppo.loss_grad_reference(**dict(b, old_neglogp=nlp + np.log(ratio)), **kw)


RUNAWAY_CASES = [(m, a) for m in (64, 257) for a in (7, 27)]
RUNAWAY_SCALE = 512.0
_cases = {}


def runaway_case(m, a, clip_value):
    """One case of the runaway loss test, computed once and shared (nobody writes to it): (batch, PPOConfig, reference, the reference's
    non-finite rows)."""
    from isaacgym_amd import ppo
    if (m, a, clip_value) not in _cases:
        b = runaway_batch(np.random.default_rng(1000 * m + a), m, a)
        cfg = ppo.PPOConfig(entropy_coef=0.01, clip_value=clip_value)
        ref = loss_grad_reference_f32_ratio(b, e_clip=cfg.e_clip, critic_coef=cfg.critic_coef, bounds_loss_coef=cfg.bounds_loss_coef,
                                            entropy_coef=cfg.entropy_coef, clip_value=clip_value, scale=RUNAWAY_SCALE)
        _cases[m, a, clip_value] = (b, cfg, ref, nonfinite_rows(ref["d_mu"], ref["d_value"]))
    return _cases[m, a, clip_value]


def log_ratio(b):
    return b["old_neglogp"].astype(np.float64) - neglogp64(b["actions"], b["mu"], b["logstd"])


def assert_runaway_margins(b, e_clip=0.2, margin=1e-3):
    """On the fp64 reference's own quantities: no row within `margin` of a switch an fp32 rounding could take the other way (the ratio against
    1 +- e where it is near them at all; |v - old_v| against e; the two value losses, relatively: they reach 1e6), and every kind of row present."""
    f = lambda k: b[k].astype(np.float64)
    c = log_ratio(b)
    near = np.abs(c) < 1.0
    ratio = np.exp(c[near])
    assert np.abs(ratio - (1 + e_clip)).min() > margin and np.abs(ratio - (1 - e_clip)).min() > margin
    d = f("value") - f("old_values")
    assert np.abs(np.abs(d) - e_clip).min() > margin
    vc = f("old_values") + np.clip(d, -e_clip, e_clip)
    cu, cc = (f("value") - f("returns")) ** 2, (vc - f("returns")) ** 2
    out = np.abs(d) > e_clip
    assert (np.abs(cu - cc)[out] > 1e-5 * np.maximum(cu, cc)[out]).all()
    assert (np.abs(d) < e_clip).any() and (np.abs(d) > 30).any() and (cu > cc).any() and (cu < cc).any()
    adv = f("advantages")
    assert (np.abs(adv[adv != 0]) >= 0.05).all() and (adv > 0).any() and (adv < 0).any()
    assert (adv == 0).any() and (np.abs(c[adv == 0]) < 1.0).all()
    with np.errstate(over="ignore"):
        r32 = np.exp(c).astype(F32)
    tiny = np.finfo(F32).tiny
    for what, rows in (("0", r32 == 0), ("denormal", (r32 > 0) & (r32 < tiny)), ("normal", (r32 >= tiny) & np.isfinite(r32) & ~near),
                       ("inf in fp32 only", np.isinf(r32) & (c < 709)), ("inf in fp64", c > 710)):
        assert rows.any(), f"no row with a ratio that is {what}"


def nonfinite_rows(d_mu, d_value):
    """The rows whose fp32 image of d_mu / d_value holds an inf or a NaN (the kernel writes fp32: a value beyond its range is an inf there)."""
    with np.errstate(all="ignore"):
        return ~(np.isfinite(np.asarray(d_mu).astype(F32)).all(1) & np.isfinite(np.asarray(d_value).astype(F32)))
