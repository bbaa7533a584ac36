"""Actuator usage accounting on the MI355X (isaacgym_amd.play: ActuatorStats, Player(actuators=...); include/ppenv_play_act.h).

The kernels against their host build (tests/csrc/play_act_shim.cpp, which sums in the kernels' order) on the cases the host tests run:
running state, totals and the launch's partials BYTE FOR BYTE after every step, run to run, and through a captured graph.  Then the Player
on three tasks: its report is the one built from the host build's totals when that is fed the tensors the test cloned every step; the
option changes nothing else of the result; swept cells differ and equal cells do not.  The tasks run with env.episodeLength 12.
Need a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import play_act_shim_binding as pa
from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (two fixtures, two helpers)

pytestmark = pytest.mark.gpu

T3, TT, TN = "HumanoidPingpongG1", "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNoEarlyStopG1"
TA, T4 = "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
N_ENVS = 130
THR = dict(zip(("effort_frac", "vel_frac", "limit_margin", "action_clip"), pa.THRESHOLDS))


def device_pack(torch, layout, q, qd, tau, action):
    """pa.pack's buffers on the device, and the four tensors ActuatorStats.accumulate takes: [N, D] views of them."""
    views, bufs = pa.pack(layout, q, qd, tau, action)
    dev = [None if b is None else torch.from_numpy(b).to(DEV) for b in bufs]
    if layout == "soa":
        return [dev[0].T, dev[1].T, dev[2].T, dev[3]]
    return [dev[0][:, :, 0], dev[0][:, :, 1], dev[1], dev[2]]


def partial_totals(raw, G, parts, D):
    """The launch's partials (ActuatorStats.partial_bytes() or HostAct.partial) as bytes per group: what play_act_totals_kernel reads."""
    ng, nj = C.sizeof(pa.PlayActGroup), C.sizeof(pa.PlayActJoint)
    return [(raw[g * parts * ng:(g + 1) * parts * ng], raw[G * parts * ng + g * parts * D * nj:G * parts * ng + (g + 1) * parts * D * nj]) for g in range(G)]


# ------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("case", pa.CASES, ids=pa.case_id)
def test_kernels_match_shim_byte_for_byte_after_every_step(torch_cuda, case):
    torch = torch_cuda
    from isaacgym_amd.play import ActuatorStats
    S, (D, A), layout, with_action = case
    G, games_num, parts = pa.GROUPS, pa.games_num_of(S), (S + pa.BLOCK - 1) // pa.BLOCK
    q, qd, tau, action, dones = pa.streams(S, A, D)
    shim = pa.HostAct(S, G, A, D, games_num, pa.case_limits(D), pa.THRESHOLDS)
    runs = [ActuatorStats(S, G, D, games_num, pa.case_limits(D), THR, DEV, num_agents=A) for _ in range(2)]
    for st in runs:
        for t in st._state, st._group, st._joint, st._partial:                               # garbage: reset() must clear it
            t.fill_(0x55)
        st.reset()
    d_dev = torch.from_numpy(dones).to(DEV)
    for s in range(pa.STEPS):
        a = action[s] if with_action else None
        views, keep = pa.pack(layout, q[s], qd[s], tau[s], a)
        frozen = [int(g.games) >= games_num for g in shim.read()[0]]
        shim.accumulate(*views, dones[s])
        ins = device_pack(torch, layout, q[s], qd[s], tau[s], a)
        for st in runs:
            st.accumulate(*ins, d_dev[s])
        want = shim.state_bytes()
        assert runs[0].state_bytes() == want, (pa.case_id(case), s)                         # running state, group totals, joint totals
        assert runs[1].state_bytes() == want                                                 # run to run
        got_p, want_p = partial_totals(runs[0].partial_bytes(), G, parts, D), partial_totals(shim.partial.tobytes(), G, parts, D)
        for g in range(G):                                                                   # a frozen group's partials are not written (nor read)
            assert frozen[g] or got_p[g] == want_p[g], (pa.case_id(case), s, g)
    groups, joints = pa.read_totals(*runs[0].state_bytes()[1:], G, D)
    assert int(groups[0].launches) < pa.STEPS == int(groups[1].launches) and int(groups[0].games) >= games_num > int(groups[1].games) > 0
    got = runs[0].read()
    assert [t["games"] for t in got] == [int(g.games) for g in groups] and got[0]["abs_tau"] == [j.abs_tau for j in joints[0]]


def test_accumulate_refuses_wrong_tensors(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.play import ActuatorStats
    S, G, D = 5, 2, 7
    st = ActuatorStats(S, G, D, 3, pa.case_limits(D), THR, DEV)
    x, done = torch.zeros((S * G, D), device=DEV), torch.zeros(S * G, dtype=torch.int64, device=DEV)
    st.accumulate(x, x, x, None, done)
    st.accumulate(x.T.contiguous().T, x, x, x.reshape(-1), done)                              # strided view; contiguous in another shape
    for bad in (dict(q=x[:-1]), dict(qd=x.double()), dict(tau=x.cpu()), dict(action=x[:, :-1]), dict(done=done.int()), dict(done=done[:-1])):
        args = dict(q=x, qd=x, tau=x, action=x, done=done)
        args.update(bad)
        with pytest.raises(ValueError, match="accumulate"):
            st.accumulate(**args)
    assert [t["launches"] for t in st.read()] == [2, 2]


def test_captured_accumulate_replayed_equals_eager_calls(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.play import ActuatorStats
    S, (D, A) = 65, (27, 1)
    G, games_num = pa.GROUPS, pa.games_num_of(S)
    q, qd, tau, action, dones = pa.streams(S, A, D)
    eager, graphed = (ActuatorStats(S, G, D, games_num, pa.case_limits(D), THR, DEV, num_agents=A) for _ in range(2))
    states, force, act = (torch.zeros(shape, dtype=torch.float32, device=DEV) for shape in ((S * G, D, 2), (S * G, D), (S * G, D)))
    stage = [states[:, :, 0], states[:, :, 1], force, act]                                   # fixed addresses: the graph reads these
    done = torch.zeros(S * G * A, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream(DEV)
    warm = ActuatorStats(S, G, D, games_num, pa.case_limits(D), THR, DEV, num_agents=A)
    with torch.cuda.stream(side):
        warm.accumulate(*stage, done)                                                        # warm-up on the capture stream, on another state
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    graphed.reset()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        graphed.accumulate(*stage, done)
    graphed.reset()                                                                          # (a capture launches nothing; start from zero anyway)
    for s in range(pa.STEPS):
        states.copy_(torch.from_numpy(np.ascontiguousarray(np.stack([q[s], qd[s]], axis=2))).to(DEV))
        force.copy_(torch.from_numpy(tau[s]).to(DEV))
        act.copy_(torch.from_numpy(action[s]).to(DEV))
        done.copy_(torch.from_numpy(dones[s]).to(DEV))
        eager.accumulate(*stage, done)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
    assert graphed.state_bytes() == eager.state_bytes()
    assert sum(t["games"] for t in eager.read()) > 0 and eager.read()[0]["launches"] < pa.STEPS


# ------------------------------------------------------------------------------------------------------- the Player
def env_tensors(task):
    """Clones of the env's joint tensors as float32 numpy [N, D] views: q, qd, tau."""
    env = task.env
    if hasattr(env, "dof_states"):
        st, f = env.dof_states.clone().cpu().numpy(), env.dof_force_tensor.clone().cpu().numpy()
        return st[:, :, 0], st[:, :, 1], f
    return tuple(t.clone().cpu().numpy().T for t in (env.dof_pos, env.dof_vel, env.dof_force))


@pytest.mark.parametrize("name", [TT, T4, TA])
def test_player_report_is_the_host_builds(torch_cuda, checkpoint, name):
    torch = torch_cuda
    from isaacgym_amd import play
    games_num = 400                                                                          # some four episodes of every env
    pl = play.Player(make_plain(name, N_ENVS, 21), load_policy(checkpoint(name if name != T4 else TT)), games_num=games_num, actuators=True)
    task, A = pl.task, pl.num_agents
    limits, names = play.actuator_limits(task)
    D = len(names)
    assert D == {TT: 7, T4: 14, TA: 27}[name] and pl.act.thresholds == dict(play.ACT_THRESHOLDS, action_clip=float(task.clip_actions))
    shim = pa.HostAct(N_ENVS, 1, A, D, games_num, limits, [pl.act.thresholds[k] for k in THR])
    pl.start()
    for step in range(200):
        pl.step()
        torch.cuda.synchronize()
        q, qd, tau = env_tensors(task)
        act = pl.actions.clone().cpu().numpy().reshape(N_ENVS, D)
        shim.accumulate(q, qd, tau, act, task.reset_buf.clone().cpu().numpy())
        if step % 8 == 7 and pl.stats.read()["games"] >= games_num:
            break
    totals = pl.stats.read()
    assert totals["games"] >= games_num and step < 199
    assert pl.act.state_bytes() == shim.state_bytes()                                        # running state and totals, byte for byte
    groups, joints = shim.read()
    want = play.act_totals_dict(groups[0], joints[0])
    assert pl.act.read() == [want]
    rep = pl.read_actuators()
    dt = play.control_dt_of(task)
    assert rep == dict(thresholds=pl.act.thresholds, joints=names, control_dt=dt, total=play.actuator_summary(want, limits, names, dt),
                       groups=[dict(cell={}, **play.actuator_summary(want, limits, names, dt))])
    assert rep["total"]["games"] == totals["games"] and rep["total"]["samples"] == totals["steps"] - totals["games"] > 0
    assert rep["total"]["energy_per_game"] > 0.0 and rep["total"]["mean_power"] > 0.0 and len(rep["total"]["per_joint"]) == D
    if name != TA:                                                                           # the 7-dof drive clamps its torque at the effort limit
        assert all(j["tau_peak"] <= float(limits[d][2]) and j["tau_peak_frac"] <= 1.0 for d, j in enumerate(rep["total"]["per_joint"]))
    assert any(j["tau_peak"] > 0.0 and j["vel_peak"] > 0.0 for j in rep["total"]["per_joint"])


def without(res, *keys):
    return {k: v for k, v in res.items() if k not in keys + ("seconds",)}


@pytest.mark.parametrize("name", [T3, TT, TN, T4, TA])
def test_the_option_changes_nothing_else(torch_cuda, checkpoint, name):
    from isaacgym_amd.play import Player
    path = checkpoint(name if name in (TT, TA) else TT)
    kw = dict(games_num=40, poll_every=16, max_steps=2000)
    off = Player(make_plain(name, N_ENVS, 21), load_policy(path), **kw).run()
    on = Player(make_plain(name, N_ENVS, 21), load_policy(path), actuators=dict(effort_frac=0.5), **kw).run()
    assert "actuators" not in off and without(on, "actuators") == without(off)
    act = on["actuators"]
    assert act["thresholds"]["effort_frac"] == 0.5 and act["thresholds"]["vel_frac"] == 0.98 and len(act["groups"]) == 1 and act["groups"][0]["cell"] == {}
    assert act["total"]["games"] == on["games"] and act["total"]["samples"] == round(on["av_steps"] * on["games"]) - on["games"]


def test_the_option_changes_nothing_else_with_a_sweep(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    sweep = Sweep.grid({"link_mass_scale": [0.7, 1.3]})
    kw = dict(games_num=30, poll_every=16, max_steps=2000, sweep=sweep)
    off = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), **kw).run()
    on = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), actuators=True, **kw).run()
    assert without(on, "actuators") == without(off) and on["groups"] == off["groups"]
    act = on["actuators"]
    assert [g["cell"] for g in act["groups"]] == [{"link_mass_scale": 0.7}, {"link_mass_scale": 1.3}]
    assert [g["games"] for g in act["groups"]] == [g["games"] for g in on["groups"]] and act["total"]["games"] == on["games"]
    assert act["total"]["samples"] == sum(g["samples"] for g in act["groups"])


def test_cli_prints_a_table_per_cell_and_writes_the_report(torch_cuda, checkpoint, capsys, tmp_path):
    import json
    from isaacgym_amd import play
    out = tmp_path / "act.json"
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "129", "--games", "20", "--poll-every", "16", "--seed", "3", "--max-steps", "1500",
                     "--actuators", "--sweep", "link_mass_scale=0.7,1.0,1.3", "--vel-frac", "0.5", "--actuators-out", str(out)])
    lines = capsys.readouterr().out.splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith("actuators cell link_mass_scale=")]
    assert len(heads) == 3 and lines[heads[1]].startswith("actuators cell link_mass_scale=1: games ")
    for h in heads:                                                                          # a column line, then one row per joint
        assert "at eff" in lines[h + 1] and [l.split()[0] for l in lines[h + 2:h + 9]] == res["actuators"]["joints"]
    written = json.loads(out.read_text())
    assert written == res["actuators"] and written["thresholds"]["vel_frac"] == 0.5 and written["thresholds"]["effort_frac"] == 0.98
    assert [g["cell"] for g in written["groups"]] == [{"link_mass_scale": v} for v in (0.7, 1.0, 1.3)] and f"wrote {out}" in lines


def test_swept_cells_differ_and_equal_cells_do_not(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    kw = dict(games_num=30, poll_every=16, max_steps=2000, actuators=True)
    res = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), sweep=Sweep.grid({"link_mass_scale": [0.7, 1.3]}, paired=True), paired_diff=True, **kw).run()
    a, b = (without(g, "cell") for g in res["actuators"]["groups"])
    assert a != b and a["per_joint"] != b["per_joint"] and res["paired_diff"]["complete"]
    same = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), sweep=Sweep([{}, {}], paired=True), **kw).run()
    a, b = same["actuators"]["groups"]
    assert a == b and a["games"] >= 30
