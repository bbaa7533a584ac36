"""Actuator usage accounting (include/ppenv_play_act.h) without a GPU: the kernel bodies on the host (tests/csrc/play_act_shim.cpp) against
a numpy restatement of the header's rule, the freeze, the thresholds to the ulp, the games against the episode accounting's on the same
done stream, the C entries' refusals, and the Python side: the limits table, the summary arithmetic, the CLI options."""
import ctypes as C
import json
import math
import os
import subprocess
import types

import numpy as np
import pytest

import play_act_shim_binding as pa
import play_shim_binding as ps
from isaacgym_amd import _lib, play, scene
from isaacgym_amd._lib import PlayActGroup, PlayActInput, PlayActInputs, PlayActJoint, PlayActThresholds

EINVAL = -1
_HERE = os.path.dirname(os.path.abspath(__file__))


def _run_case(case, on_step=None):
    """The shim over one shared case -> (HostAct, the streams, games per group after every step by the shim)."""
    S, (D, A), layout, with_action = case
    q, qd, tau, action, dones = pa.streams(S, A, D)
    h = pa.HostAct(S, pa.GROUPS, A, D, pa.games_num_of(S), pa.case_limits(D), pa.THRESHOLDS)
    games = []
    for s in range(pa.STEPS):
        views, keep = pa.pack(layout, q[s], qd[s], tau[s], action[s] if with_action else None)
        h.accumulate(*views, dones[s])
        games.append([int(g.games) for g in h.read()[0]])
        if on_step is not None:
            on_step(s, h)
    return h, (q, qd, tau, action if with_action else None, dones), games


@pytest.mark.parametrize("case", pa.CASES, ids=pa.case_id)
def test_shim_equals_the_numpy_restatement(case):
    S, (D, A), layout, with_action = case
    h, (q, qd, tau, action, dones), games = _run_case(case)
    games_np, want, n_np = pa.numpy_act(q, qd, tau, action, dones, S, pa.GROUPS, A, D, pa.games_num_of(S), pa.case_limits(D), pa.THRESHOLDS)
    assert games == games_np                                                     # after every step
    groups, joints = h.read()
    pa.check_totals(groups, joints, want, pa.case_id(case))
    assert np.array_equal(h.state[:S * pa.GROUPS].view(np.int32), n_np)
    # the case does what it is for: group 0 froze mid-stream, group 1 never did, and somebody folded a game without a sample
    assert want[0]["launches"] < pa.STEPS and want[0]["games"] >= pa.games_num_of(S)
    assert want[1]["launches"] == pa.STEPS and 0 < want[1]["games"] < pa.games_num_of(S)
    if not with_action:
        assert all(int(j.c_clip) == 0 for J in joints for j in J)
    else:
        assert sum(int(j.c_clip) for J in joints for j in J) > 0
    assert sum(int(j.c_effort) for J in joints for j in J) > 0 and sum(int(j.c_vel) for J in joints for j in J) > 0
    assert sum(int(j.c_limit) for J in joints for j in J) > 0 and max(j.max_exc for J in joints for j in J) > 0.0


@pytest.mark.parametrize("case", [c for c in pa.CASES if c[2] == "aos" and c[3]], ids=pa.case_id)
def test_games_and_samples_against_the_episode_accounting(case):
    """The same done stream through play_shim_binding's accounting, group by group: games agree after EVERY step, and at the end
    samples == steps - games, where `steps` is the accounting's sum of the finished games' lengths."""
    S, (D, A), _, _ = case
    _, _, _, _, dones = pa.streams(S, A, D)
    ref = [ps.HostStats(S, A, pa.games_num_of(S)) for _ in range(pa.GROUPS)]
    rew = np.zeros(S * A, np.float32)

    def on_step(s, h):
        for g, r in enumerate(ref):
            r.accumulate(rew, dones[s].reshape(pa.GROUPS, S * A)[g])
            assert r.read()["games"] == int(h.read()[0][g].games), (s, g)

    h, _, _ = _run_case(case, on_step)
    for g, r in enumerate(ref):
        t, mine = r.read(), h.read()[0][g]
        assert int(mine.samples) == t["steps"] - t["games"] and int(mine.launches) == t["launches"]


def test_a_frozen_group_stops_changing_while_the_others_go_on():
    case = (65, (27, 1), "aos", True)
    S, (D, A), _, _ = case
    snaps = []
    _run_case(case, lambda s, h: snaps.append(h.state_bytes()))
    ng, nj, N = C.sizeof(PlayActGroup), C.sizeof(PlayActJoint), S * pa.GROUPS

    def of(snap, g):
        state = np.frombuffer(snap[0], np.uint32).reshape(-1, N)[:, g * S:(g + 1) * S]
        return state.tobytes(), snap[1][g * ng:(g + 1) * ng], snap[2][g * D * nj:(g + 1) * D * nj]

    games0 = [PlayActGroup.from_buffer_copy(of(s, 0)[1]).games for s in snaps]
    first = next(i for i, g in enumerate(games0) if g >= pa.games_num_of(S))
    assert first < pa.STEPS - 5
    for s in snaps[first + 1:]:
        assert of(s, 0) == of(snaps[first], 0)
    assert of(snaps[-1], 1) != of(snaps[first], 1) and of(snaps[-1], 2) != of(snaps[first], 2)


def test_a_game_of_length_one_folds_no_sample_and_the_state_is_zero_after_a_fold():
    D = 3
    h = pa.HostAct(1, 1, 1, D, 100, pa.case_limits(D), pa.THRESHOLDS)
    x = np.full((1, D), 0.5, np.float32)
    h.accumulate(x, x, x, x, np.array([1], np.int64))                          # done in the very first step: a game of length 1
    (g,), (J,) = h.read()
    assert (g.games, g.samples, g.launches, g.energy, g.energy_sq) == (1, 0, 1, 0.0, 0.0)
    assert all(j.abs_tau == 0.0 and j.max_abs_tau == 0.0 and j.max_exc == -math.inf and j.c_limit == 0 for j in J)
    h.accumulate(x, x, x, x, np.array([0], np.int64))
    h.accumulate(x, 2 * x, 3 * x, x, np.array([0], np.int64))
    assert h.state[0] == 2 and not np.all(h.state == 0)
    h.accumulate(9 * x, 9 * x, 9 * x, 9 * x, np.array([1 << 32], np.int64))  # not sampled: the 9s appear nowhere
    (g,), (J,) = h.read()
    assert (g.games, g.samples, g.launches) == (2, 2, 4) and np.all(h.state == 0)
    E = np.float32(0.0)
    for d in range(D):
        E = np.float32(E + np.float32(np.float32(0.25) + np.float32(1.5)))      # |0.5 * 0.5| + |1.5 * 1.0| per dof
    assert g.energy == float(E) and g.energy_sq == float(E) ** 2
    assert all(j.abs_tau == 2.0 and j.tau_sq == 2.5 and j.power == 1.75 and j.max_abs_tau == 1.5 and j.max_abs_vel == 1.0 for j in J)
    assert [j.max_exc for j in J] == [np.float32(0.5) - np.float32(u) for u in pa.case_limits(D)[:, 1]]


def test_values_on_a_threshold_count_and_one_ulp_below_do_not():
    f32, below = np.float32, lambda v: np.nextafter(np.float32(v), np.float32(0.0))
    limits = np.array([[-8.0, 1.0, 25.0, 37.0]] * 2, np.float32)
    thr = (0.98, 0.97, 0.25, 1.0)
    eff, vel = f32(0.98) * f32(25.0), f32(0.97) * f32(37.0)
    #              dof 0: exactly on every threshold       dof 1: one ulp below each
    tau = np.array([[-eff, below(eff)]], np.float32)
    qd = np.array([[vel, -below(vel)]], np.float32)
    q = np.array([[0.75, below(0.75)]], np.float32)                            # exc = q - upper = -0.25 = -limit_margin, or an ulp less
    act = np.array([[-1.0, below(1.0)]], np.float32)
    h = pa.HostAct(1, 1, 1, 2, 5, limits, thr)
    h.accumulate(q, qd, tau, act, np.array([0], np.int64))
    h.accumulate(q, qd, tau, act, np.array([2], np.int64))
    (_,), (J,) = h.read()
    assert [(j.c_effort, j.c_vel, j.c_limit, j.c_clip) for j in J] == [(1, 1, 1, 1), (0, 0, 0, 0)]
    low = pa.HostAct(1, 1, 1, 2, 5, limits, thr)                                # the lower limit's side of the same test
    ql = np.array([[-7.75, -below(7.75)]], np.float32)
    low.accumulate(ql, qd, tau, None, np.array([0], np.int64))
    low.accumulate(ql, qd, tau, None, np.array([1], np.int64))
    assert [(j.c_limit, j.c_clip) for j in low.read()[1][0]] == [(1, 0), (0, 0)]


# ------------------------------------------------------------------------------------------------------- the C entries
SIZES = "num_dofs outside 1..32 or no multiple of num_agents, groups outside 1..1024, envs_per_group <= 0, num_agents not 1 or 2, or more than 2^31 - 1 rows"
RESET_TEXT = f"pp_play_act_reset: NULL pointer, {SIZES}"
ACC_TEXT = f"pp_play_act_accumulate: NULL pointer, {SIZES}, or games_num < 1"
P = 0x1000                      # a non-NULL pointer value: a refusal comes before anything is read or launched


def _poison(L):
    assert L.ppenv_gae(*([None] * 2 + [0, 0, None, 0, 0, 0.0, 0.0, 0.0, None, None, None])) == EINVAL      # another text in ppenv_last_error()
    return L.ppenv_last_error().decode()


def _inputs(action=True, **null):
    one = lambda name: PlayActInput(None if null.get(name) else P, 1, 1)
    return PlayActInputs(one("q"), one("qd"), one("tau"), PlayActInput(P if action else None, 1, 1))


def _acc(L, ins=None, done=P, S=4, G=2, A=1, D=7, games=5, limits=P, thr=True, state=P, group=P, joint=P, partial=P):
    t = PlayActThresholds(0.98, 0.98, 0.02, 1.0)
    return L.pp_play_act_accumulate(C.byref(ins) if ins is not None else None, done, S, G, A, D, games, limits, C.byref(t) if thr else None, state, group, joint,
                                    partial, None)


def test_entries_are_bound_on_the_default_library_and_on_one_loaded_by_path(tmp_path):
    import shutil
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    for L in (_lib.lib(), _lib.load(str(shutil.copy(_lib.LIB_PATH, tmp_path / "libppenv_copy.so")))):
        for fn in (L.pp_play_act_state_bytes, L.pp_play_act_partial_bytes):
            assert fn.argtypes == [i32, i32, i32] and fn.restype is C.c_size_t
        assert L.pp_play_act_reset.argtypes == [i32, i32, i32, vp, vp, vp, vp]
        assert L.pp_play_act_accumulate.argtypes == [C.POINTER(PlayActInputs), vp, i32, i32, i32, i32, i64, vp, C.POINTER(PlayActThresholds), vp, vp, vp, vp, vp]
    assert not [n for n in vars(_lib.lib()) if n.startswith("ppenv_play_act")]             # the pinned set of ppenv_* symbols is untouched
    for name in ("ppenv_play_act_reset", "ppenv_play_act_accumulate", "ppenv_play_act_state_bytes", "ppenv_play_act_partial_bytes"):
        assert not hasattr(C.CDLL(_lib.LIB_PATH), name)                                  # ... nor does the library export one


def test_state_and_partial_bytes():
    L = _lib.lib()
    for S, G, D, parts in ((1, 1, 7, 1), (256, 1, 14, 1), (257, 1, 27, 2), (300, 3, 27, 6), (63, 1024, 32, 1024), (4096, 16, 1, 256)):
        assert L.pp_play_act_state_bytes(S, G, D) == 4 * (1 + 10 * D) * S * G
        assert L.pp_play_act_partial_bytes(S, G, D) == parts * (40 + 72 * D)
    for S, G, D in ((0, 1, 7), (-1, 1, 7), (1, 0, 7), (1, 1025, 7), (1 << 30, 2, 7), (4, 2, 0), (4, 2, 33), (4, 2, -1)):
        assert L.pp_play_act_state_bytes(S, G, D) == 0 and L.pp_play_act_partial_bytes(S, G, D) == 0


@pytest.mark.parametrize("S,G,D", [(0, 1, 7), (-5, 1, 7), (4, 0, 7), (4, -1, 7), (4, 1025, 7), (4, 2, 0), (4, 2, 33), (1 << 21, 1024, 7)])
def test_reset_refuses_sizes(S, G, D):
    L = _lib.lib()
    assert _poison(L) != RESET_TEXT
    assert L.pp_play_act_reset(S, G, D, P, P, P, None) == EINVAL
    assert L.ppenv_last_error().decode() == RESET_TEXT


def test_reset_refuses_null():
    L = _lib.lib()
    for k in range(3):
        _poison(L)
        assert L.pp_play_act_reset(4, 2, 7, *[None if i == k else P for i in range(3)], None) == EINVAL
        assert L.ppenv_last_error().decode() == RESET_TEXT


@pytest.mark.parametrize("kw", [dict(S=0), dict(S=-3), dict(G=0), dict(G=1025), dict(A=0), dict(A=3), dict(D=0), dict(D=33), dict(D=7, A=2), dict(S=1 << 21, G=1024),
                                dict(S=1 << 20, G=1024, A=2, D=14), dict(games=0), dict(games=-3)], ids=str)
def test_accumulate_refuses_sizes(kw):
    L = _lib.lib()
    assert _poison(L) != ACC_TEXT
    assert _acc(L, _inputs(), **kw) == EINVAL
    assert L.ppenv_last_error().decode() == ACC_TEXT


@pytest.mark.parametrize("kw", [dict(ins=None), dict(ins=_inputs(q=True)), dict(ins=_inputs(qd=True)), dict(ins=_inputs(tau=True)), dict(done=None), dict(limits=None),
                                dict(thr=False), dict(state=None), dict(group=None), dict(joint=None), dict(partial=None)], ids=lambda kw: next(iter(kw)))
def test_accumulate_refuses_null(kw):
    L = _lib.lib()
    _poison(L)
    kw.setdefault("ins", _inputs())
    assert _acc(L, **kw) == EINVAL
    assert L.ppenv_last_error().decode() == ACC_TEXT


# ------------------------------------------------------------------------------------------------------- the Python side
def test_python_refusals():
    for kw in (dict(envs_per_group=0), dict(groups=0), dict(groups=1025), dict(num_dofs=0), dict(num_dofs=33), dict(games_num=0), dict(num_agents=3),
               dict(num_dofs=7, num_agents=2), dict(limits=np.zeros((6, 4)))):
        args = dict(envs_per_group=4, groups=2, num_dofs=7, games_num=5, limits=np.zeros((7, 4)), thresholds=dict(zip(("effort_frac", "vel_frac", "limit_margin",
                    "action_clip"), pa.THRESHOLDS)), device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match="ActuatorStats"):
            play.ActuatorStats(**args)


def test_actuator_limits_reproduces_the_config_numbers():
    cfg = scene.build_config("TT", num_envs=4)
    table, names = scene.joint_limits(cfg, 1)
    assert table.dtype == np.float32 and table.shape == (scene.NUM_DOF, 4) and len(names) == scene.NUM_DOF
    for d, j in enumerate(cfg.joint):
        assert list(table[d]) == [np.float32(j.lower), np.float32(j.upper), np.float32(j.effort), np.float32(j.vel_limit)]
    assert names[0] == "right_shoulder_pitch_joint" and all(n.endswith("_joint") for n in names)
    assert [float(v) for v in table[0, 2:]] == [scene.G1_RIGHT_ARM[0]["effort"], scene.G1_RIGHT_ARM[0]["vel"]]
    t4, n4 = scene.joint_limits(scene.build_config("T4", num_envs=4), 2)
    assert t4.shape == (14, 4) and np.array_equal(t4[:7], t4[7:]) and np.array_equal(t4[:7], table)
    assert n4[:7] == ["h1/" + n for n in names] and n4[7:] == ["h2/" + n for n in names]
    model = scene.build_ta_model()
    model.link[5].effort = 123.5                                                # a model of the caller's: ITS numbers, not the stock ones
    ta, na = scene.ta_joint_limits(model)
    assert ta.shape == (scene.TA_NUM_DOF, 4) and ta[4, 2] == np.float32(123.5)
    for d in range(scene.TA_NUM_DOF):
        k = model.link[d + 1]
        assert list(ta[d]) == [np.float32(k.lower), np.float32(k.upper), np.float32(k.effort), np.float32(k.vel_limit)]
    from isaacgym_amd import urdf
    assert na == urdf.ta_dof_joint_names()
    from isaacgym_amd.env import PPEnv
    assert PPEnv.control_dt.fget(types.SimpleNamespace(config=cfg)) == float(cfg.dt)        # the 7-dof env's control_dt on this config
    env = types.SimpleNamespace(control_dt=float(cfg.dt), joint_limits=lambda: (table, names))
    got = play.actuator_limits(types.SimpleNamespace(env=env))
    assert play.control_dt_of(types.SimpleNamespace(env=env)) == float(cfg.dt) and got[0] is table and got[1] is names


def _totals(games, samples, D=2, scale=1.0):
    return dict(games=games, samples=samples, launches=samples + games, energy=10.0 * scale * games, energy_sq=(110.0 * scale * scale) * games,
                c_effort=[samples // 2, 0], c_vel=[1, 0], c_limit=[0, samples], c_clip=[samples // 4, 0], abs_tau=[2.0 * samples, 1.0 * samples],
                tau_sq=[9.0 * samples, 4.0 * samples], power=[5.0 * samples, 0.5 * samples], max_abs_tau=[25.0, 3.0 * scale], max_abs_vel=[37.0, 1.0],
                max_exc=[-0.5, 0.125 * scale])


def test_summary_arithmetic_and_json_round_trip(tmp_path):
    limits, names = np.array([[-1, 1, 25, 37], [-2, 2, 50, 20]], np.float32), ["a_joint", "b_joint"]
    a, b = _totals(4, 40), _totals(2, 16, scale=2.0)
    ea = play.actuator_summary(a, limits, names, 0.0125)
    assert ea["games"] == 4 and ea["samples"] == 40 and ea["energy_per_game"] == 0.0125 * 40.0 / 4 and ea["mean_power"] == 1.0
    assert ea["energy_stderr"] == pytest.approx(0.0125 * math.sqrt((440.0 - 1600.0 / 4) / 3 / 4), rel=1e-15)
    j0, j1 = ea["per_joint"]
    assert j0 == dict(joint="a_joint", tau_mean_abs=2.0, tau_rms=3.0, tau_peak=25.0, tau_peak_frac=1.0, at_effort=0.5, vel_peak=37.0, vel_peak_frac=1.0,
                      at_vel_limit=1 / 40, at_pos_limit=0.0, excursion_max=-0.5, power_mean=5.0, action_clip=0.25)
    assert j1["at_pos_limit"] == 1.0 and j1["excursion_max"] == 0.125 and j1["tau_peak_frac"] == 3.0 / 50.0 and j1["vel_peak_frac"] == 0.05
    tot = play.sum_act_totals([a, b])
    assert tot["games"] == 6 and tot["samples"] == 56 and tot["energy"] == 80.0 and tot["c_limit"] == [0, 56] and tot["abs_tau"] == [112.0, 56.0]
    assert tot["max_abs_tau"] == [25.0, 6.0] and tot["max_exc"] == [-0.5, 0.25]
    empty = play.actuator_summary(dict(_totals(0, 0), max_exc=[-math.inf] * 2), limits, names, 0.0125)
    assert empty["games"] == 0 and all(math.isnan(empty[k]) for k in ("energy_per_game", "energy_stderr", "mean_power"))
    assert math.isnan(empty["per_joint"][0]["at_effort"]) and empty["per_joint"][0]["excursion_max"] == -math.inf
    one = play.actuator_summary(_totals(1, 9), limits, names, 0.0125)
    assert math.isnan(one["energy_stderr"]) and one["energy_per_game"] == 0.125
    report = dict(thresholds=dict(zip(("effort_frac", "vel_frac", "limit_margin", "action_clip"), pa.THRESHOLDS)), joints=names, control_dt=0.0125,
                  total=play.actuator_summary(tot, limits, names, 0.0125),
                  groups=[dict(cell={"link_mass_scale": 0.7}, **ea), dict(cell={"link_mass_scale": 1.3}, **play.actuator_summary(b, limits, names, 0.0125))])
    path = tmp_path / "act.json"
    path.write_text(json.dumps(report, indent=1))
    assert json.loads(path.read_text()) == report
    text = play.actuator_table(report["groups"][0], "cell link_mass_scale=0.7")
    lines = text.splitlines()
    assert len(lines) == 2 + len(names) and lines[0].startswith("actuators cell link_mass_scale=0.7: games 4 samples 40 energy/game 0.125 +- ")
    assert lines[2].split()[0] == "a_joint" and lines[3].split()[0] == "b_joint" and "at eff" in lines[1]


def test_act_totals_dict_reads_the_structs():
    g = PlayActGroup(3, 30, 33, 1.5, 2.25)
    J = [PlayActJoint(1, 2, 3, 4, 5.0, 6.0, 7.0, 8.0, 9.0, -math.inf, 0.0), PlayActJoint(0, 0, 0, 0, 0.5, 0.25, 0.125, 1.0, 2.0, 0.5, 0.0)]
    assert play.act_totals_dict(g, J) == dict(games=3, samples=30, launches=33, energy=1.5, energy_sq=2.25, c_effort=[1, 0], c_vel=[2, 0], c_limit=[3, 0],
                                              c_clip=[4, 0], abs_tau=[5.0, 0.5], tau_sq=[6.0, 0.25], power=[7.0, 0.125], max_abs_tau=[8.0, 1.0],
                                              max_abs_vel=[9.0, 2.0], max_exc=[-math.inf, 0.5])


def test_cli_options():
    base = ["--checkpoint", "x.pth"]
    a = play.parse_args(base)
    assert a.actuators is False and a.actuators_out is None and play.actuator_option(a) is False
    a = play.parse_args(base + ["--actuators"])
    assert a.actuators is True and play.actuator_option(a) is True
    a = play.parse_args(base + ["--actuators", "--effort-frac", "0.9", "--limit-margin", "0.05", "--actuators-out", "act.json", "--sweep", "link_mass_scale=0.7:1.3:3"])
    assert play.actuator_option(a) == dict(effort_frac=0.9, limit_margin=0.05) and a.actuators_out == "act.json" and a.vel_frac is None
    assert play.actuator_option(play.parse_args(base + ["--actuators", "--vel-frac", "0.5"])) == dict(vel_frac=0.5)
    for extra in (["--actuators-out", "act.json"], ["--effort-frac", "0.9"], ["--vel-frac", "0.9"], ["--limit-margin", "0.1"]):
        with pytest.raises(SystemExit):
            play.parse_args(base + extra)
    assert play.actuator_option(types.SimpleNamespace()) is False                  # a hand-made namespace of before the option


# ------------------------------------------------------------------------------------------------------- the shim under sanitizers
def test_shim_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (tests/csrc/play_act_sanitize_main.cpp: the shim plus a main over one case per layout, every buffer sized as
    the ABI says), built with -fsanitize=address,undefined and run on its own; never loaded into Python."""
    exe = tmp_path / "play_act_sanitize"
    src = os.path.join(_HERE, "csrc", "play_act_sanitize_main.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                    "-o", str(exe), src], check=True, capture_output=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    assert res.stdout.count("games") == 9
