"""The loss scale's rule and the runaway rows of tests/test_ppo_runaway_gpu.py, on the host (no GPU): the numpy restatement of the scaler
rule (ppo_reference.scaler_update; include/ppenv_ppo.h) against a hand-written table of transitions at both limits, the shares of finite and
non-finite rows the fp64 reference gives in every case of the runaway loss test, and — in a numpy float32 restatement of the Adam kernel's
element update — why the rule exists: without it a scale halved below fp32's normal range turns a gradient of exactly 0 into a NaN."""
import numpy as np
import pytest

import ppo_reference as R
from ppo_reference import CONSTANT, DYNAMIC, F32, scaler_state, scaler_steps, scaler_update

DENORM_MIN = float(np.finfo(np.float32).smallest_subnormal)
INF, NAN = float("inf"), float("nan")

# (hp, state before: scale, growth_tracker, step, skipped, floor_hits; finite; state after) — written by hand from include/ppenv_ppo.h
TABLE = [
    # the healthy middle: torch's GradScaler.update
    (DYNAMIC, (1024.0, 0, 5, 0, 0), True, (1024.0, 1, 6, 0, 0)),
    (DYNAMIC, (1024.0, 2, 5, 0, 0), True, (2048.0, 0, 6, 0, 0)),
    (DYNAMIC, (1024.0, 2, 5, 1, 0), False, (512.0, 0, 5, 2, 0)),
    # the floor
    (DYNAMIC, (2.0, 1, 5, 7, 0), False, (1.0, 0, 5, 8, 0)),                 # reached, not crossed: the floor changed nothing
    (DYNAMIC, (1.0, 0, 5, 8, 0), False, (1.0, 0, 5, 9, 1)),                 # held
    (DYNAMIC, (1.0, 0, 5, 9, 1), False, (1.0, 0, 5, 10, 2)),
    (DYNAMIC, (1.0, 2, 5, 9, 1), True, (2.0, 0, 6, 9, 1)),                  # and left again by growth
    (DYNAMIC, (1.5, 0, 5, 0, 0), False, (1.0, 0, 5, 1, 1)),                 # 0.75 -> 1
    # states below the floor (a checkpoint of a run that had none): lifted by a clean update, and by a skipped one
    (DYNAMIC, (2.0 ** -100, 0, 5, 150, 0), True, (1.0, 1, 6, 150, 1)),
    (DYNAMIC, (2.0 ** -100, 2, 5, 150, 0), True, (1.0, 0, 6, 150, 1)),      # growth first (2^-99), then the floor
    (DYNAMIC, (2.0 ** -100, 0, 5, 150, 0), False, (1.0, 0, 5, 151, 1)),
    (DYNAMIC, (2.0 ** -126, 0, 5, 150, 0), True, (1.0, 1, 6, 150, 1)),      # the smallest normal number: its reciprocal 2^126 is finite
    # nothing finite divides these out: the step is skipped even on finite gradients
    (DYNAMIC, (2.0 ** -127, 1, 5, 143, 0), True, (1.0, 0, 5, 144, 1)),
    (DYNAMIC, (DENORM_MIN, 1, 5, 166, 0), True, (1.0, 0, 5, 167, 1)),
    (DYNAMIC, (0.0, 1, 5, 167, 0), True, (1.0, 0, 5, 168, 1)),
    (DYNAMIC, (0.0, 1, 5, 167, 0), False, (1.0, 0, 5, 168, 1)),
    (DYNAMIC, (-4.0, 1, 5, 0, 0), True, (1.0, 0, 5, 1, 1)),
    (DYNAMIC, (NAN, 1, 5, 0, 0), True, (1.0, 0, 5, 1, 1)),
    # the top: growth is withheld where the product is inf, and the tracker restarts all the same
    (DYNAMIC, (2.0 ** 126, 2, 5, 0, 0), True, (2.0 ** 127, 0, 6, 0, 0)),
    (DYNAMIC, (2.0 ** 127, 1, 5, 0, 0), True, (2.0 ** 127, 2, 6, 0, 0)),
    (DYNAMIC, (2.0 ** 127, 2, 5, 0, 0), True, (2.0 ** 127, 0, 6, 0, 0)),
    (DYNAMIC, (2.0 ** 127, 2, 5, 0, 0), False, (2.0 ** 126, 0, 5, 1, 0)),
    (DYNAMIC, (INF, 0, 5, 0, 0), False, (INF, 0, 5, 1, 0)),                 # out of the rule's reach: growth can no longer produce it
    # a constant scale (mixed_precision: False): never changed, never lifted
    (CONSTANT, (1.0, 2, 5, 0, 0), True, (1.0, 0, 6, 0, 0)),
    (CONSTANT, (1.0, 2, 5, 0, 0), False, (1.0, 0, 5, 1, 0)),
    (CONSTANT, (0.25, 1, 5, 0, 0), False, (0.25, 0, 5, 1, 0)),
    (CONSTANT, (0.25, 1, 5, 0, 0), True, (0.25, 2, 6, 0, 0)),
    (CONSTANT, (0.0, 1, 5, 0, 0), True, (0.0, 0, 5, 1, 0)),                 # skipped (0 x inf otherwise), but the caller's constant stays
]


def _same(got, want):
    for k, w in zip(R.SCALER_FIELDS, want):
        g = got[k]
        if not (g == w or (k == "scale" and np.isnan(g) and np.isnan(w))):
            return False
    return isinstance(got["scale"], np.float32)


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_scaler_rule_matches_the_hand_written_table(row):
    hp, before, finite, after = TABLE[row]
    got = scaler_update(scaler_state(*before), finite, hp)
    assert _same(got, after), (before, finite, got, after)
    assert scaler_steps(scaler_state(*before), finite) == (after[2] == before[2] + 1)


def test_scaler_rule_over_long_bursts():
    """200 skipped steps from the default 65536 end at the floor after 16 and stay; 400 clean steps from 2^120 at growth_interval 3 stop at
    2^127 after 21."""
    st, scales = scaler_state(65536.0), []
    for _ in range(200):
        st = scaler_update(st, False, DYNAMIC)
        scales.append(float(st["scale"]))
    assert scales[:16] == [2.0 ** (15 - k) for k in range(16)] and set(scales[16:]) == {1.0}
    assert (st["skipped"], st["step"], st["floor_hits"]) == (200, 0, 184)
    st, scales = scaler_state(2.0 ** 120), []
    for _ in range(400):
        st = scaler_update(st, True, DYNAMIC)
        scales.append(float(st["scale"]))
    assert scales[2] == 2.0 ** 121 and scales[20] == 2.0 ** 127 and max(scales) == 2.0 ** 127 and np.isfinite(scales).all()
    assert (st["skipped"], st["step"], st["growth_tracker"]) == (0, 400, 400 % 3)


@pytest.mark.parametrize("clip_value", [True, False])
@pytest.mark.parametrize("m,a", R.RUNAWAY_CASES)
def test_runaway_reference_has_finite_and_nonfinite_rows(m, a, clip_value):
    """Every case of the GPU test: the rows clear every switch, hold every kind of ratio, and the fp64 reference (ratio rounded to fp32, outputs
    read as fp32) gives at least 10 % finite and at least 5 % non-finite rows."""
    b, cfg, ref, bad = R.runaway_case(m, a, clip_value)
    R.assert_runaway_margins(b, cfg.e_clip)
    print(f"  m={m} a={a} clip_value={clip_value}: finite rows {(~bad).mean():.3f}, non-finite rows {bad.mean():.3f}")
    assert (~bad).mean() >= 0.10 and bad.mean() >= 0.05
    # the non-finite rows are the ones the construction names — a negative advantage under a ratio that is inf in fp32 — and those whose
    # gradient, finite in fp64, is beyond fp32's range
    with np.errstate(over="ignore"):
        inf_ratio = np.isinf(np.exp(R.log_ratio(b)).astype(F32)) & (b["advantages"] < 0)
    assert (bad[inf_ratio]).all()
    assert np.isfinite(ref["d_mu"][bad & ~inf_ratio]).all() and np.isfinite(ref["d_value"]).all()
    for k in ("c_loss", "b_loss", "entropy", "kl", "clip_frac"):
        assert np.isfinite(ref[k]), k
    assert not np.isfinite(ref["loss"]) and not np.isfinite(ref["a_loss"]) and not np.isfinite(ref["d_logstd"]).any()


def test_f32_ratio_wrapper_changes_only_the_ratio():
    """On healthy rows (test_ppo_gpu._batch's log ratios) the wrapper is ppo.loss_grad_reference up to the ratio's fp32 rounding, 2^-24."""
    from isaacgym_amd import ppo
    rng = np.random.default_rng(5)
    m, a = 64, 7
    old_v = rng.standard_normal(m)
    b = R.rows_around(rng, rng.uniform(-1.6, 1.6, (m, a)), rng.uniform(-2.2, -1.5, a), rng.choice(R.HEALTHY_C, m), rng.standard_normal(m),
                      old_v + rng.choice([-0.5, -0.1, 0.1, 0.5], m), old_v, rng.standard_normal(m))
    plain, wrapped = ppo.loss_grad_reference(**b, scale=512.0), R.loss_grad_reference_f32_ratio(b, scale=512.0)
    for k in plain:
        np.testing.assert_allclose(wrapped[k], plain[k], rtol=2.0 ** -23, atol=2.0 ** -23 * np.abs(plain[k]).max(), err_msg=k)
    assert any(not np.array_equal(wrapped[k], plain[k]) for k in plain)


# ---- why the rule exists: the Adam kernel's element update without it ---------------------------------------------------------------------
def adam1_f32(p, m, v, g, gmul, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """csrc/ppenv_ppo.hip's adam1 in numpy float32, rounding for rounding (fl(a x b + c) through fp64, exact for fp32 operands up to the final
    rounding); gmul: the unscale-and-clip factor."""
    fma = lambda a, b, c: F32(np.float64(a) * np.float64(b) + np.float64(c))
    with np.errstate(all="ignore"):
        g = F32(g) * F32(gmul)
        m = fma(F32(1.0 - beta1), g - F32(m), F32(m))
        v = fma(F32(1.0 - beta2) * g, g, F32(v) * F32(beta2))
        denom = np.sqrt(v) / F32(np.sqrt(1.0 - beta2 ** step)) + F32(eps)
        p = fma(-F32(lr / (1.0 - beta1 ** step)), m / denom, F32(p))
    return p, m, v


def reciprocal_f32(scale, flush_denormals):
    """1.0f / scale: IEEE, or with a denormal operand read as 0 (what a reciprocal that flushes denormals gives)."""
    scale = F32(scale)
    if flush_denormals and abs(scale) < np.finfo(F32).tiny:
        scale = F32(0.0)
    with np.errstate(all="ignore"):
        return F32(1.0) / scale


def test_unbounded_scale_turns_a_zero_gradient_into_nan():
    """The unfixed kernel: gmul = (1 / scale) x coef on every clean step.  From the default 65536, 143 halvings reach 2^-127 and 144 reach
    2^-128; there the scaled gradients have underflowed to exactly 0 — finite, so the step is taken — and 0 x inf is NaN in the parameter and
    both moments.  With denormal operands flushed that is 2^-127; in IEEE arithmetic 1 / 2^-127 = 2^127 is the last finite reciprocal and
    the NaN comes one halving later.  Either way torch's unbounded rule gets there, and the bounded rule never does: it refuses every scale
    below 2^-126 before the reciprocal is formed."""
    scale = F32(65536.0)
    for _ in range(143):
        scale = scale * F32(0.5)
    assert scale == F32(2.0 ** -127)
    assert np.isinf(reciprocal_f32(scale, flush_denormals=True)) and reciprocal_f32(scale, flush_denormals=False) == F32(2.0 ** 127)
    assert all(np.isnan(x) for x in adam1_f32(0.3, 0.01, 1e-4, 0.0, reciprocal_f32(scale, True)))
    assert all(np.isfinite(x) for x in adam1_f32(0.3, 0.01, 1e-4, 0.0, reciprocal_f32(scale, False)))
    below = scale * F32(0.5)                                  # 2^-128: no arithmetic has a finite reciprocal for it
    for flush in (True, False):
        assert all(np.isnan(x) for x in adam1_f32(0.3, 0.01, 1e-4, 0.0, reciprocal_f32(below, flush)))
    # with truncate and a gradient norm beyond fp32 the clip coefficient is 0, and inf x 0 is the same NaN as a factor
    with np.errstate(invalid="ignore"):
        gmul = reciprocal_f32(below, False) * F32(0.0)
    assert all(np.isnan(x) for x in adam1_f32(0.3, 0.01, 1e-4, 1e-40, gmul))
    # the bounded rule: none of these scales steps, every one that steps has a finite reciprocal under either arithmetic
    for s in (scale, below, DENORM_MIN, 0.0):
        assert not scaler_steps(scaler_state(s), True)
    for s in (2.0 ** -126, 2.0 ** -100, 1.0, 2.0 ** 127):
        assert scaler_steps(scaler_state(s), True)
        for flush in (True, False):
            assert all(np.isfinite(x) for x in adam1_f32(0.3, 0.01, 1e-4, 0.0, reciprocal_f32(s, flush)))
