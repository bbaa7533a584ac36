"""The scripted states of tests/reward_branch_scenarios.py: stepped by the oracle alone they reach every cell of the reward and reset decision
of TT, TN, T3 and T4 (compute_reward / compute_reward_side2, csrc/ppenv_device.h) at least FLOOR times, in the plain pass and in the reset
pass, with at most 2 % of the env-steps set aside; the thresholds and cells the module states are the oracle's; then the kernels' arithmetic on
the host (ShimEnv) against the oracle on them.  The same comparison runs on the HIP kernels in tests/test_reward_branches_gpu.py."""
import numpy as np
import pytest

import ball_contact_scenarios as sc
import reward_branch_scenarios as rs
import shim_binding as sb
from helpers import ExclusionLog, golden_config, load_golden, reward_atol
from isaacgym_amd import scene

SEED = 1
# Scanned with the oracle alone in steps of one case cycle (TT by 47, TN by 38, T3 by 22, T4 by 94): the smallest size that holds both floors in both
# passes.  The slices MARGIN .. 2 MARGIN beside each threshold set it: a slice is half a case.  None is a multiple of 64.
SIZES = {"TT": 815, "TN": 343, "T3": 166, "T4": 1535}
TIMEOUT_FLOOR = 2            # env-steps of every cell that time out in the reset pass: 3 envs in 7 do, a cell at the floor expects 3.4

f32 = np.float32
PASSES = [(v, r) for v in rs.VARIANTS for r in (False, True)]


@pytest.fixture(scope="module", params=PASSES, ids=[f"{v}-{'reset_pass' if r else 'plain_pass'}" for v, r in PASSES])
def run(request, oracle_lib):
    variant, resets = request.param
    assert SIZES[variant] % 64
    return variant, resets, rs.oracle_run(variant, SIZES[variant], SEED, resets)


def test_every_reward_cell_holds_the_floor(run):
    variant, resets, r = run
    kept, before = rs.cell_counts(r), rs.cell_counts(r, kept=False)
    timed = rs.cell_counts(r, only_timeouts=True) if resets else {}
    for name in rs.cells_of(variant, resets):
        print(f"[{variant}, resets={resets}] {name:44s} {kept[name]:5d} kept of {before[name]}" + (f", {timed[name]} of them time out" if resets else ""))
    low = {k: v for k, v in kept.items() if v < rs.FLOOR}
    assert not low, f"[{variant}, resets={resets}] cells under the floor of {rs.FLOOR} kept env-steps: {low}"
    if resets:
        alone = {k: v for k, v in timed.items() if v < TIMEOUT_FLOOR and k != "timeout/one_step_short" and k not in rs.NOT_WITH_TIMEOUT}
        assert not alone, f"[{variant}] cells that share fewer than {TIMEOUT_FLOOR} env-steps with a time-out: {alone}"


def test_set_aside_share_is_under_the_bound(run):
    variant, resets, r = run
    n = SIZES[variant]
    aside, near = sum(int((~s["keep"]).sum()) for s in r.steps), sum(int(s["near"].sum()) for s in r.steps)
    unknown = sum(int((~s["terms"]["known"]).sum()) for s in r.steps)
    print(f"[{variant}, resets={resets}] set aside {aside} of {n * rs.STEPS} env-steps ({100 * aside / (n * rs.STEPS):.3f} %), {near} of them by near_threshold; "
          f"{unknown} died after a contact and are in the death cells alone")
    assert aside <= rs.EXCLUDED_BOUND * n * rs.STEPS
    assert unknown <= rs.EXCLUDED_BOUND * n * rs.STEPS


def test_discrete_terms_are_reached_through_their_constants():
    """REACHED x the reward tolerance: every constant a cell pays, in the configs the suites run and in the golden task configs."""
    for variant in rs.VARIANTS:
        cfgs = [scene.build_config(variant, num_envs=4, seed=rs.ENV_SEED)]
        if variant != "T4":                                    # (the 4-actor task has no yaml of its own: build_config's values are its task config)
            cfgs.append(golden_config(variant, load_golden(variant)))
        for cfg in cfgs:
            ra = (2 if cfg.num_humanoids == 2 else 1) * reward_atol(cfg)
            terms = {"penalty": cfg.penalty}
            if variant in ("TT", "T4"):
                terms.update(hit_table_reward=cfg.hit_table_reward, not_hit_table_penalty=cfg.not_hit_table_penalty, net=rs.NET_REWARD)
            if variant == "TN":
                terms.update(floor=rs.TN_FLOOR_REWARD)
                assert rs.TN_POS_REACHED * ra <= 1.0 < rs.REACHED * ra      # the named exception: pos_reward <= 1 cannot be REACHED x the tolerance
            for name, v in terms.items():
                assert abs(float(v)) >= rs.REACHED * ra, (variant, name, v, ra)


# ------------------------------------------------------------------------------------------------------------------ the thresholds are the oracle's
def _evaluate(oracle_lib, variant, side, rows):
    """The oracle's reward function on hand-made tensors (its tensor-API entry points; no physics): rows = dicts of bx, by, bz, vx, pre_vx, flags,
    px (the blade's x).  -> [(reward, reset, flag word after)] per row."""
    m = len(rows)
    get = lambda k, d: np.array([r.get(k, d) for r in rows])
    if variant == "T4":
        p = scene.build_t4_params(m)
        rb, root = np.zeros((m, 82, 13), np.float32), np.zeros((m, 4, 13), np.float32)
        cfg = scene.build_config("T4", num_envs=m, seed=rs.ENV_SEED)
        root[:, 0, 0], root[:, 1, 0] = cfg.humanoid_root_pos[0], cfg.humanoid2_root_pos[0]
        rb[:, 39, 0], rb[:, 79, 0] = get("px", 0.4), get("px", 3.1)
        rb[:, (39, 79), 2] = 1.1
        for k, col in (("bx", 0), ("by", 1), ("bz", 2), ("vx", 7)):
            root[:, 3, col] = get(k, 0.0)
        fl = get("flags", rs.NB).astype(np.uint32)
        out = oracle_lib.t4_rewards(p, rb, root, np.zeros((m, 14, 2), np.float32), np.zeros((m, 14), np.float32), get("pre_vx", 0.0).astype(np.float32),
                                    np.full(m, 5, np.int64), fl.copy(), fl.copy())
        return list(zip(out[side].tolist(), out[2 + side].tolist(), out[4 + side].tolist()))
    cfg = scene.build_config(variant, num_envs=m, seed=rs.ENV_SEED)
    o = oracle_lib.OracleEnv(cfg)
    rb, root = np.zeros((m, scene.NUM_BODIES, 13), np.float32), np.zeros((m, scene.NUM_ACTORS, 13), np.float32)
    root[:, 0, 0] = cfg.humanoid_root_pos[0]
    rb[:, 39, 0], rb[:, 39, 2] = get("px", 0.4), 1.1
    for k, col in (("bx", 0), ("by", 1), ("bz", 2), ("vx", 7)):
        root[:, 2, col] = get(k, 0.0)
    o.flags[:], o.progress_buf[:] = get("flags", rs.NB).astype(np.uint32), 5
    o.post_physics_step(rb, root, np.zeros((m, 7, 2), np.float32), np.zeros((m, 7), np.float32), get("pre_vx", 0.0).astype(np.float32))
    out = list(zip(o.rew_buf.tolist(), o.reset_buf.tolist(), o.flags.tolist()))
    o.close()
    return out


# (variants, side, base point, the coordinate, the module's threshold, which neighbour the value AT the threshold behaves as)
_FAR = dict(bx=2.8, by=0.0, bz=0.8, vx=2.0, pre_vx=1.0)
_NET = dict(bx=1.75, by=0.0, bz=1.05, vx=2.0, pre_vx=1.0)
_BACK = dict(bx=-0.3, by=0.7, bz=1.2, vx=-2.0, pre_vx=-2.0)
_MIRROR = lambda d: dict(d, bx=3.5 - d["bx"], by=-d["by"], vx=-d["vx"], pre_vx=-d["pre_vx"])
THRESHOLDS = []
for _vs, _side, _mir in ((("TT", "T4"), 0, lambda d: d), (("T4",), 1, _MIRROR)):
    _lo, _hi = ("below", "above") if _side == 0 else ("above", "below")
    THRESHOLDS += [(_vs, _side, _mir(b), k, thr, at) for b, k, thr, at in (
        (_FAR, "bx", rs.X_HALF[_side], "neither"), (_FAR, "bx", rs.X_END[_side], _hi), (_FAR, "bz", rs.Z_BOUNCE, "above"),
        (_FAR, "by", rs.Y_BOUNCE, "above"), (_FAR, "by", -rs.Y_BOUNCE, "below"), (_FAR, "vx", f32(0.0), _lo),
        (dict(_FAR, pre_vx=-1.0), "pre_vx", f32(0.0), _hi),
        (_NET, "bx", rs.NET_X[0], "below"), (_NET, "bx", rs.NET_X[1], "above"), (_NET, "by", rs.NET_Y, "above"), (_NET, "by", -rs.NET_Y, "below"),
        (_NET, "bz", rs.NET_Z[0], "below"), (_NET, "bz", rs.NET_Z[1], "above"), (_NET, "vx", f32(0.0), _lo),
        (dict(_FAR, bx=3.3, bz=0.5), "bz", rs.Z_DIE, "above"),
        (_BACK, "bx", f32(0.0) - rs.BACK if _side == 0 else f32(3.5) + rs.BACK, _hi))]
THRESHOLDS += [(("TN",), 0, dict(bx=1.5, by=0.0, bz=1.0, vx=2.0, pre_vx=-1.0), "vx", rs.TN_HIT_VX, "below"),
               (("TN",), 0, dict(_BACK, px=-0.5), "bx", f32(0.0) - rs.BACK, "above"),
               (("TN",), 0, dict(_BACK, bx=0.2, px=0.4), "bx", f32(0.4) - rs.TN_PADDLE_BACK, "above"),
               (("TN", "T3"), 0, dict(bx=3.3, by=0.0, bz=0.5, vx=2.0, pre_vx=1.0), "bz", rs.Z_DIE, "above"),
               (("T3",), 0, dict(bx=1.0, by=0.0, bz=1.2, vx=-2.0, pre_vx=-2.0, px=0.4), "bx", f32(0.4) - rs.T3_PADDLE_BACK, "above"),
               # (T3's vx > 0 pays alpha |vx|, nothing at the smallest positive vx, and sets no bit: it is not measurable this way)
               (("T3",), 0, dict(bx=1.0, by=0.0, bz=1.2, vx=2.0, pre_vx=-2.0), "pre_vx", f32(0.0), "above")]


def test_thresholds_are_the_oracles(oracle_lib):
    """Every threshold the module states switches the ORACLE's reward function exactly there: the fp32 neighbours below and above the value give
    different outputs (reward, reset or flag word), and the value itself goes with the side the module's comparison (< or <=) puts it on."""
    for variants, side, base, key, thr, at in THRESHOLDS:
        thr = f32(thr)
        below, above = np.nextafter(thr, f32(-np.inf), dtype=np.float32), np.nextafter(thr, f32(np.inf), dtype=np.float32)
        for variant in variants:
            lo, mid, hi = _evaluate(oracle_lib, variant, side, [dict(base, **{key: float(v)}) for v in (below, thr, above)])
            what = f"{variant} side {side + 1}: {key} at {thr!r} from {base}"
            # (the continuous terms move with the coordinate's last bit: rewards are the same where they differ by less than 1e-3, every discrete term is 200 or more)
            same = lambda a, b: abs(a[0] - b[0]) < 1e-3 and a[1:] == b[1:]
            assert not same(lo, hi), f"{what}: the oracle does not switch here ({lo})"
            assert {"below": same(mid, lo), "above": same(mid, hi), "neither": not same(mid, lo) and not same(mid, hi)}[at], f"{what}: below {lo}, at {mid}, above {hi}"


# ------------------------------------------------------------------------------------------------------------------ the cells are the oracle's
# cell -> (the sticky bit that gates it, the term the oracle's reward loses when the bit is set instead of clear; a callable takes (cfg, terms))
_vel = lambda cfg, t: abs(float(cfg.alpha_velocity_reward)) * np.abs(t["vx"].astype(np.float64))
_TT_TERMS = {"vel_reward/paid": (rs.CC, _vel), "early/paid": (rs.RC, lambda cfg, t: float(cfg.not_hit_table_penalty)),
             "good/paid": (rs.RC, lambda cfg, t: float(cfg.hit_table_reward)), "beyond/paid": (rs.RC, lambda cfg, t: float(cfg.not_hit_table_penalty))}
GATED_TERMS = {"TT": _TT_TERMS, "T4": _TT_TERMS, "T3": {},
               "TN": {"vel_reward/paid": (rs.CC, _vel), "penalty/paid": (rs.MC, lambda cfg, t: float(cfg.penalty))}}


def test_cells_are_what_the_oracle_pays(run, oracle_lib):
    """classify against the oracle's own behaviour: stepped again from the same state with a paid cell's gating bit SET, the oracle's reward is
    smaller by that cell's term, on the cell's env-steps; where NO_BOUNCE decides (good/paid against good/refused), by hit_table_reward with the bit
    cleared.  The flag words the cells promise: `early` leaves NO_BOUNCE clear and REWARD_CALC set, TN's floor term resets nobody, a turn at no more
    than 1 m/s leaves TN's COND_CALC clear, T3 pays a turn whatever COND_CALC says and leaves the word alone."""
    variant, resets, r = run
    cfg, A, n = r.cfg, r.num_agents, SIZES[variant]
    o = oracle_lib.OracleEnv(cfg, threads=8)
    ra = (2 if A == 2 else 1) * reward_atol(cfg)
    checked = 0
    for s in r.steps:
        t, main = s["terms"], s["main"]
        rew, flags1 = main.rew_buf.reshape(n, A).astype(np.float64), main.flags.reshape(A, n)
        stays = main.reset_buf.reshape(n, A)[:, 0] == 0
        for a in range(A):
            pre = "h2/" if a else ""
            gated = dict(GATED_TERMS[variant])
            if variant in ("TT", "T4"):
                gated["good/refused_no_bounce_clear"] = (rs.NB, lambda cfg, t: -float(cfg.hit_table_reward))     # toggling SETS the bit here: the reward gains
            for cell, (bit, term) in gated.items():
                m = s["cells"][pre + cell] & s["keep"]
                if not m.any():
                    continue
                o.set_state(s["st"])
                o.flags.reshape(A, n)[a, m] ^= np.uint32(bit)
                o.step(s["act"])
                lost = rew[m, a] - o.rew_buf.reshape(n, A)[m, a]
                want = np.broadcast_to(term(cfg, {k: (v[m] if isinstance(v, np.ndarray) else v) for k, v in t.items()}), lost.shape)
                # (TN's COND_CALC closes pos_reward <= 1 with the same bit)
                np.testing.assert_allclose(lost, want, rtol=1e-5, atol=ra + (1.0 if variant == "TN" and bit == rs.CC else 0.0), err_msg=f"[{variant}] {pre}{cell}")
                checked += int(m.sum())
            if variant in ("TT", "T4"):
                for cell in ("early/paid", "early/gated_reward_calc"):
                    m = s["cells"][pre + cell] & stays
                    assert ((flags1[a, m] & (rs.NB | rs.RC)) == rs.RC).all(), f"[{variant}] {pre}{cell}: NO_BOUNCE must be clear and REWARD_CALC set afterwards"
                for cell in ("beyond/vx_not_positive_sets_flag", "beyond/exactly_at"):
                    m = s["cells"][pre + cell] & stays
                    assert ((flags1[a, m] & rs.RC) != 0).all(), f"[{variant}] {pre}{cell}"
        if variant == "TN":
            assert not main.reset_buf[s["cells"]["floor/on"] & (s["progress_after"] < cfg.max_episode_length - 1)].any()
            assert ((flags1[0, s["cells"]["hit_paddle/vx_at_most_1"] & stays] & rs.CC) == 0).all()
        if variant == "T3":
            np.testing.assert_array_equal(flags1[0, stays], np.asarray(s["flags0"]).reshape(A, n)[0, stays])
            m = s["cells"]["vel_reward/paid_cond_calc_set"] | s["cells"]["vel_reward/paid"]
            o.set_state(s["st"])
            o.flags[m] ^= np.uint32(rs.CC)
            o.step(s["act"])
            np.testing.assert_array_equal(o.rew_buf[m], main.rew_buf[m])
            checked += int(m.sum())
    o.close()
    assert checked > 0


def test_what_the_reward_saw_is_on_record(run):
    """terms(): the oracle with the ball parked has the watching oracle's bodies wherever that one did not reset (the ball does not move the arm); the
    fp64 free flight ends where the watching oracle's ball does wherever it met nothing and nobody died; in the reset pass the envs with env % 7 = 3 end the
    run at max_episode_length - 2 after the increment, not reset by it, next to those that time out in the last step."""
    variant, resets, r = run
    cfg, A, n = r.cfg, r.num_agents, SIZES[variant]
    for s in r.steps:
        t, w = s["terms"], s["watch"]
        alive = ~t["died"]
        for a in range(A):
            np.testing.assert_array_equal(t["paddle"][a][alive], t["watch_rb"][alive, scene.NUM_HUMANOID_BODIES * a + 39, :3])
        free = alive & t["free_flight"]
        np.testing.assert_allclose(w.ball[0:3][:, free].T, t["p_end"][free], rtol=0, atol=1e-6)
        assert free.sum() > n // 2
    if resets:
        last, L, env = r.steps[-1], int(cfg.max_episode_length), np.arange(n)
        short = (env % 7 == 3) & ~np.any([s["terms"]["died"] for s in r.steps], axis=0)
        assert short.sum() >= rs.FLOOR
        rows = lambda x: x.reshape(n, A)[:, 0]
        assert (rows(last["main"].progress_buf)[short] == L - 2).all() and not rows(last["main"].reset_buf)[short].any()
        out = (env % 7 == 2) & ~np.any([s["terms"]["died"] for s in r.steps[:-1]], axis=0)
        assert rows(last["main"].reset_buf)[out].all() and (rows(last["main"].progress_buf)[out] == 0).all()
        assert (last["main"].flags.reshape(A, n)[:, out] == rs.NB).all()


def test_named_exceptions_stay_unreachable(run):
    """UNREACHABLE's other entries, so that they fail once a scenario reaches them: no env-step has the ball exactly on X_END or X_HALF while it moves
    towards that side's far end (there the >= of the penalty at X_END and the strict comparisons at X_HALF would show; the exactly placed balls have vx = 0,
    which `bounce` and the penalty refuse), and no T3 env turns in two steps of a run."""
    variant, resets, r = run
    turns = 0
    for s in r.steps:
        t = s["terms"]
        if variant in ("TT", "T4"):
            for a in range(r.num_agents):
                sg = 1.0 if a == 0 else -1.0
                on = (t["bx"] == rs.X_END[a]) | (t["bx"] == rs.X_HALF[a])
                assert not (on & (sg * t["vx"] > 0)).any(), f"[{variant}] side {a + 1}: a moving ball exactly on a threshold: give it a cell"
        if variant == "T3":
            turns = turns + ((t["pre_vx"] < 0) & (t["vx"] > 0))
    if variant == "T3":
        assert turns.max() == 1, "a T3 env turns twice in one run: give it a cell"
    assert len(rs.UNREACHABLE) == 3


def test_t4_sides_reset_together(oracle_lib):
    """UNREACHABLE["T4: exactly one side's reset fires"]: the oracle's two reward functions, called on what the run's rewards saw (every ball of
    both passes, the time-outs and the deaths among them), never disagree about the reset."""
    checked = 0
    for resets in (False, True):
        r = rs.oracle_run("T4", SIZES["T4"], SEED, resets)
        n = SIZES["T4"]
        p = scene.build_t4_params(n, episode_length=int(r.cfg.max_episode_length))
        for s in r.steps:
            t = s["terms"]
            k = t["known"]
            rb, root = np.zeros((n, 82, 13), np.float32), np.zeros((n, 4, 13), np.float32)
            root[:, 0, 0], root[:, 1, 0] = r.cfg.humanoid_root_pos[0], r.cfg.humanoid2_root_pos[0]
            rb[:, 39, :3], rb[:, 79, :3] = t["paddle"]
            for key, col in (("bx", 0), ("by", 1), ("bz", 2), ("vx", 7)):
                root[:, 3, col] = np.nan_to_num(t[key], nan=1.0)
            f = np.asarray(s["flags0"]).reshape(2, n)
            out = oracle_lib.t4_rewards(p, rb, root, np.zeros((n, 14, 2), np.float32), np.zeros((n, 14), np.float32), t["pre_vx"].copy(),
                                        s["progress_after"].astype(np.int64), f[0].copy(), f[1].copy())
            np.testing.assert_array_equal(out[2][k], out[3][k])
            np.testing.assert_array_equal(out[2][k], s["main"].reset_buf.reshape(n, 2)[k, 0])
            assert out[2][k].any() and not out[2][k].all()
            checked += int(k.sum())
    assert checked > SIZES["T4"]


# ------------------------------------------------------------------------------------------------------------------ the kernels' arithmetic
def test_kernel_arithmetic_on_every_reward_cell(run, oracle_lib):
    """ppenv_device.h compiled for the host (fp32), restarted from the oracle's state each step, against the oracle: rew_buf per actor within
    reward_atol, reset_buf, progress_buf, the flag word per actor and episode exactly, the observation row and the state (after a reset: the whole
    re-initialised state) at the suite's tolerances; the set-aside env-steps through check_excluded with none unmatched."""
    variant, resets, r = run
    cfg = r.cfg
    s_env = sb.ShimEnv(cfg)
    oa, ra = rs.tolerances(cfg)
    log = ExclusionLog(f"host shim (kernel arithmetic) on the scripted reward branches vs oracle [{variant}, {'reset' if resets else 'plain'} pass]", bound=rs.EXCLUDED_BOUND)
    o = oracle_lib.OracleEnv(cfg)
    for t, s in enumerate(r.steps):
        o.set_state(s["st"])
        s_env.copy_state_from(o)
        s_env.step(s["act"])
        log.add(s["keep"])
        r.probe.check_excluded(log, t, s["st"], s["act"], s["main"], s_env, s["keep"], oa, ra)
        sc.compare_step(s_env, s, t, cfg, oa, ra, f"host shim [{variant}, resets={resets}]")
    o.close()
    log.close()
