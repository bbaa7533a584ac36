"""Plain fp64 restatements (numpy, loops where a loop is the plainest form) of what PPOTrainer does between the rollout and the loss kernel:
the episode bookkeeping, GAE, the value de-normalisation and prepare().  Written from the rl_games formulas the trainer's docstrings name, not
from the torch code; tests/test_ppo_bookkeeping_host.py checks them against independent formulations on the CPU, and the GPU tests use them
as the reference."""
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
