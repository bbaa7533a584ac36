"""Reset-time domain randomisation (include/ppenv_dr.h), the part a CPU can check: the HIP kernels' per-env body
(isaacgym_amd/csrc/ppenv_dr_device.h) compiled by g++ (tests/csrc/dr_shim.cpp) against restatements written here, and the mapping of
the task yaml onto a plan.  No GPU."""
import copy

import numpy as np
import pytest

import dr_shim_binding as drs
from isaacgym_amd import scene

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("frequency", [1, 5, 1000])
def test_rule_matches_upstream_restatement(frequency):
    """Upstream VecTask.apply_randomizations' env rule + TT:1025, restated in numpy: randomize_buf += 1 every step; the first
    application redraws every env; afterwards exactly the envs with reset_buf != 0 and randomize_buf >= frequency, whose
    randomize_buf goes to 0.  randomize_buf, draws and WHICH table columns changed are equal exactly, step by step."""
    n, steps = 64, 220
    h = drs.HostDR(drs.mixed_plan(frequency=frequency), n, seed=11)
    resets = drs.scripted_resets(steps, n)
    rbuf, draws = np.zeros(n, np.int64), np.zeros(n, np.int32)
    fired_total = 0
    for t in range(steps):
        before = {k: v.copy() for k, v in h.tables.items()}
        h.apply(resets[t])
        rbuf += 1
        mask = np.ones(n, bool) if t == 0 else (resets[t] != 0) & (rbuf >= frequency)
        rbuf[mask] = 0
        draws[mask] += 1
        fired_total += int(mask.sum())
        np.testing.assert_array_equal(h.randomize_buf, rbuf, err_msg=f"randomize_buf, step {t}")
        np.testing.assert_array_equal(h.draws, draws, err_msg=f"draws, step {t}")
        changed = np.zeros(n, bool)
        for k, v in h.tables.items():
            # (constant schedule before its step: an additive term redraws to the 0 it already holds — the other four tables tell)
            changed |= np.any(v.view(np.uint32) != before[k].view(np.uint32), axis=0)
        np.testing.assert_array_equal(changed, mask, err_msg=f"columns rewritten, step {t}")
        assert int(h.count[0]) == t + 1
    if frequency == 1000:
        assert fired_total == n                      # larger than the run: the first application only
    else:
        assert fired_total > n + 100


def test_ids_variant_counts_a_listing_as_a_reset():
    """ppenv_dr_apply_ids' body: a listed env redraws when randomize_buf[e] >= frequency (or before the first step has been counted);
    randomize_buf is not incremented, the step count does not advance, ids out of range and duplicates are harmless."""
    n = 64
    h = drs.HostDR(drs.mixed_plan(frequency=3), n, seed=2)
    h.apply_ids([3, 5])                                   # nothing counted yet: first application for the listed envs only
    assert h.draws[3] == h.draws[5] == 1 and h.draws.sum() == 2 and int(h.count[0]) == 0 and not h.randomize_buf.any()
    zero = np.zeros(n, np.int64)
    for _ in range(4):
        h.apply(zero)
    assert (h.draws == np.where(np.isin(np.arange(n), [3, 5]), 2, 1)).all() and (h.randomize_buf == 3).all()      # step 1 redrew all
    before = h.tables["dof_stiffness_scale"].copy()
    h.L.dr_shim_apply_ids(drs.C.byref(h.plan), drs._p(np.array([7, -1, 64, 9], np.int64)), 4, drs._p(h.randomize_buf), drs._p(h.count), drs._p(h.draws))
    assert h.draws[7] == h.draws[9] == 2 and h.randomize_buf[7] == h.randomize_buf[9] == 0 and int(h.count[0]) == 4
    changed = np.any(h.tables["dof_stiffness_scale"] != before, axis=0)
    assert changed[[7, 9]].all() and changed.sum() == 2
    h.apply_ids([7])                                      # randomize_buf[7] = 0 < 3: not again
    assert h.draws[7] == 2


# ---------------------------------------------------------------------------------------------------------------- 2. the draws
def _hash32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def rng_uniform(seed, gid, episode, k):
    """isaacgym_amd/csrc/ppenv_device.h rng_uniform, restated."""
    h = _hash32(gid ^ (seed & 0xFFFFFFFF))
    h = _hash32(h + episode * 0x9E3779B9 + (seed >> 32))
    h = _hash32(h + (k + 1) * 0x85EBCA6B)
    return F32(h >> 8) * F32(1.0 / 16777216.0)


def sched(p, last_step):
    """isaacgym_amd/vec_task.py apply_randomizations.sched, verbatim."""
    if p.get("schedule") == "linear":
        return min(max(last_step, 0), int(p["schedule_steps"])) / float(p["schedule_steps"])
    if p.get("schedule") == "constant":
        return 1.0 if last_step > int(p["schedule_steps"]) else 0.0
    return 1.0


def sample_f32(p, base, last_step):
    """apply_randomizations.sample (vec_task.py:155-164) on a given base variate (the rand / randn value), every operand and every
    operation in float32, as torch evaluates it on a float32 tensor."""
    a, b, s = F32(p["range"][0]), F32(p["range"][1]), F32(sched(p, last_step))
    v = F32(F32(base * b) + a) if p.get("distribution", "uniform") == "gaussian" else F32(F32(base * F32(b - a)) + a)
    r = F32(F32(v * s) + F32(F32(1.0) - s)) if p.get("operation") == "scaling" else F32(v * s)
    return F32(r + F32(0.0))          # the kernel stores a zero as +0 (-0 + 0 = +0; every other value is unchanged)


def test_uniform_is_the_library_counter_rng_under_its_own_salt():
    L = drs.lib()
    for seed, gid, draw, k in [(0, 0, 0, 0), (17, 4095, 3, 129), (2 ** 40 + 5, 16384 + 77, 41, 7 * 64 + 27), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 20, 511)]:
        assert L.dr_shim_uniform(seed, gid, draw, k) == rng_uniform(seed ^ scene.DR_SEED_SALT, gid, draw, k)
    # not the serve stream (same seed, no salt) and not the noise stream (its salt)
    assert L.dr_shim_uniform(17, 5, 0, 0) != rng_uniform(17, 5, 0, 0) and L.dr_shim_uniform(17, 5, 0, 0) != rng_uniform(17 ^ 0x5DEECE66D, 5, 0, 0)


def test_gaussian_base_is_box_muller_on_the_paired_uniforms():
    """Unit normal of key k = Box-Muller on the uniforms of keys (k & ~1, k | 1): cosine branch for even k, sine for odd (the noise
    path's pairing).  Against float64 numpy.  Bound: the header's polynomials truncate below 1e-10; what is left is float32 rounding
    of the angle (|x| <= pi/4, 6e-8 relative), of the radius (<= 5.8 for a 24-bit uniform, 6e-8 relative) and of ~12 fused steps:
    below 1e-6 absolute on the product; 2e-6 asserted.  Moments of 20 000 draws: mean 0 +- 4 / sqrt(n), variance 1 +- 4 sqrt(2 / n)."""
    L = drs.lib()
    seed, sd = 99, 99 ^ scene.DR_SEED_SALT
    vals = []
    for gid in range(200):
        for k in range(100):
            u1, u2 = float(rng_uniform(sd, gid, 1, k & ~1)), float(rng_uniform(sd, gid, 1, k | 1))
            rad = np.sqrt(-2.0 * np.log(max(u1, 2.0 ** -24)))
            ref = rad * (np.sin(2 * np.pi * u2) if k & 1 else np.cos(2 * np.pi * u2))
            got = L.dr_shim_base(seed, gid, 1, k, 1)
            assert abs(got - ref) <= 2e-6, (gid, k, got, ref)
            vals.append(got)
    vals = np.asarray(vals, np.float64)
    assert abs(vals.mean()) < 4 / np.sqrt(vals.size) and abs(vals.var() - 1.0) < 4 * np.sqrt(2.0 / vals.size)


@pytest.mark.parametrize("distribution,rng_", [("uniform", (0.5, 1.5)), ("uniform", (0.0, 0.7)), ("uniform", (-0.2, 0.3)), ("gaussian", (1.0, 0.1)), ("gaussian", (0.0, 0.01))])
@pytest.mark.parametrize("operation", ["scaling", "additive"])
@pytest.mark.parametrize("schedule,schedule_steps", [(None, 0), ("linear", 3000), ("linear", 7), ("constant", 40)])
def test_values_match_the_host_policy_restatement(distribution, rng_, operation, schedule, schedule_steps):
    """distribution x operation x schedule: the kernel body's value == vec_task.py:155-164 in float32 numpy on the same base variate,
    BIT FOR BIT (the header rounds every product and sum on its own, in torch's order), at steps on both sides of every schedule's
    knee."""
    L = drs.lib()
    p = dict(distribution=distribution, operation=operation, range=rng_, schedule=schedule, schedule_steps=schedule_steps)
    en = drs.entry(distribution, operation, rng_[0], rng_[1], schedule, schedule_steps)
    for t in (0, 1, 5, 7, 8, 40, 41, 299, 3000, 3001, 10 ** 6):
        assert L.dr_shim_weight(en.schedule, en.schedule_steps, t) == F32(sched(p, t))
        for gid, draw, k in [(0, 0, 0), (63, 2, 64 + 3), (4096 + 9, 17, 2 * 64 + 27), (123456, 0, 4 * 64)]:
            base = F32(L.dr_shim_base(7, gid, draw, k, en.distribution))
            got = F32(L.dr_shim_value(drs.C.byref(en), 7, gid, draw, k, t))
            assert got.tobytes() == sample_f32(p, base, t).tobytes(), (t, gid, draw, k, got, sample_f32(p, base, t))


def test_scaling_values_agree_with_double_precision_range_arithmetic():
    """torch multiplies the float32 tensor by the PYTHON scalars (b - a), s, (1.0 - s), which are formed in double and rounded once;
    the kernel forms them from float32 a, b, s.  For the yaml's scalings that is the last bit of a value of order 1: rtol 1e-6."""
    L = drs.lib()
    for rng_ in [(0.5, 1.5), (0.7, 1.3), (0.0, 0.7)]:
        p = dict(distribution="uniform", operation="scaling", range=rng_, schedule="linear", schedule_steps=3000)
        en = drs.entry("uniform", "scaling", rng_[0], rng_[1], "linear", 3000)
        for t in (1, 299, 1500, 3000, 5000):
            s = sched(p, t)
            for k in range(40):
                u = F32(L.dr_shim_base(3, k, t, k, 0))
                ref = F32(F32(F32(u * F32(rng_[1] - rng_[0])) + F32(rng_[0])) * F32(s)) + F32(1.0 - s)
                np.testing.assert_allclose(L.dr_shim_value(drs.C.byref(en), 3, k, t, k, t), ref, rtol=1e-6, atol=0)


def test_apply_writes_the_keyed_values():
    """What a redraw stores in table i, row r, column e is the value of key k = i * 64 + r, global env id env_id_offset + e, the env's
    redraw index, at the step count including the current step — so a shard with an offset draws the columns of the whole."""
    n, off = 8, 4096
    plan = drs.mixed_plan(frequency=1)
    h = drs.HostDR(plan, n, seed=31, env_id_offset=off)
    ones = np.ones(n, np.int64)
    for step in (1, 2, 3):
        h.apply(ones)
        for i, name in enumerate(["dof_stiffness_scale", "dof_damping_scale", "link_mass_scale", "restitution_scale", "friction_scale"]):
            en = h.plan.entry[i]
            for r in range(en.rows):
                for e in (0, 5, 7):
                    want = F32(h.L.dr_shim_value(drs.C.byref(en), 31, off + e, step - 1, i * scene.DR_MAX_ROWS + r, step))
                    assert h.tables[name][r, e].tobytes() == want.tobytes(), (step, name, r, e)
    whole = drs.HostDR(plan, off + n, seed=31)
    for step in (1, 2, 3):
        whole.apply(np.ones(off + n, np.int64))
    for name in h.tables:
        np.testing.assert_array_equal(whole.tables[name][:, off:].view(np.uint32), h.tables[name].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 3. plan building
@pytest.mark.parametrize("task,dof_rows,mass_rows", [("HumanoidPingpongG1", 7, 7), ("HumanoidPingpongTiltG1", 7, 7), ("HumanoidPingpongTiltNoEarlyStopG1", 7, 7),
                                                     ("HumanoidPingpongTiltNESSparse27DOFG1", 27, 28)])
def test_golden_yaml_block_maps_to_a_plan(task, dof_rows, mass_rows):
    block = drs.task_block(task)
    plan = scene.reset_randomization_plan(block, dof_rows=dof_rows, mass_rows=mass_rows)
    assert plan["frequency"] == 600
    want = {"dof_stiffness_scale": (dof_rows, (0.5, 1.5)), "dof_damping_scale": (dof_rows, (0.5, 1.5)), "link_mass_scale": (mass_rows, (0.5, 1.5)),
            "restitution_scale": (1, (0.0, 0.7)), "friction_scale": (1, (0.7, 1.3))}
    assert set(plan["tables"]) == set(want)                       # color, lower / upper: no counterpart, ignored
    for name, (rows, rng_) in want.items():
        t = plan["tables"][name]
        assert (t["rows"], t["range"], t["distribution"], t["operation"], t["schedule"], t["schedule_steps"]) == (rows, rng_, "uniform", "scaling", "linear", 3000)
    P = scene.build_dr_plan(plan, {name: 4096 * (i + 1) for i, name in enumerate(want)}, 512, env_id_offset=1024, seed=2 ** 40 + 3, reset_rows=1)
    assert (P.num_envs, P.env_id_offset, P.seed, P.frequency, P.reset_rows, P.num_tables) == (512, 1024, 2 ** 40 + 3, 600, 1, 5)
    for i, name in enumerate(want):                               # entry order = set_randomization's argument order: it enters the RNG key
        en = P.entry[i]
        assert (en.table, en.rows, en.distribution, en.operation, en.schedule, en.schedule_steps) == (4096 * (i + 1), want[name][0], 0, 0, 1, 3000)
        assert (en.a, en.b) == (F32(want[name][1][0]), F32(want[name][1][1]))
    assert drs.C.sizeof(scene.DREntry) == 40 and drs.C.sizeof(scene.DRPlan) == 32 + 8 * 40


def test_plan_refuses_what_it_does_not_know():
    block = copy.deepcopy(drs.task_block("HumanoidPingpongTiltG1"))
    block["actor_params"]["humanoid"]["dof_properties"]["stiffness"]["distribution"] = "loguniform"
    with pytest.raises(ValueError, match="stiffness"):
        scene.reset_randomization_plan(block)
    with pytest.raises(ValueError):
        scene.build_dr_plan({"frequency": 1, "tables": {}}, {}, 4)


@pytest.mark.parametrize("task", ["HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1"])
def test_unknown_apply_at_raises_naming_the_key(task):
    from isaacgym_amd.tasks import isaacgym_task_map
    cfg = scene.default_task_cfg("TA" if "27DOF" in task else "TT")
    cfg["env"]["numEnvs"] = 4
    cfg["task"] = dict(randomize=True, randomization_params=dict(drs.task_block(task), apply_at="sometimes"))
    with pytest.raises(ValueError, match=r"task\.randomization_params\.apply_at.*sometimes"):
        isaacgym_task_map[task](cfg, "cuda:0", "cuda:0", -1, True, False, False)
