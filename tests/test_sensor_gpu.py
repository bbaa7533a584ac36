"""The sensor line on the MI355X (include/ppenv_sensor.h; isaacgym_amd.sensor.SensorLine).

pp_sensor_push on the cases the host suite shares (tests/sensor_shim_binding.py) against isaacgym_amd.sensor.reference: integers, drop
decisions, held, canaries and every s == 0 column bit-exact, the noised columns within |s| * 4 * E_MEASURED + 2^-23 * (|in| + |s g|),
E_MEASURED = 5.03e-7 being the device Box-Muller's measured error of tests/test_rng_streams_gpu.py; a captured push replayed; the noise's
moments and the drop share.  Need a real MI355X."""
import numpy as np
import pytest

import sensor_shim_binding as sb
from test_play_gpu import torch_cuda        # noqa: F401  (a fixture)
from test_rng_streams_gpu import E_MEASURED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = sb.cases()
MOMENT_SEED, DROP_SEED = 3, 3               # seeds under which sensor.reference itself is inside the two statistical bounds (checked below as well)


def phased(torch, words, phase, fill=sb.CANARY):
    """A device buffer of uint32 words (as int32) beginning `phase` words past a 16-byte boundary, one 16-byte piece of guard on either side
    -> (backing int32 tensor, the [words] view).  torch's allocations are at least 256-byte aligned."""
    back = torch.full((words + 12,), np.uint32(fill).astype(np.int32).item(), dtype=torch.int32, device=DEV)
    assert back.data_ptr() % 16 == 0
    return back, back[4 + phase:4 + phase + words]


def f32(t):
    import torch
    return t.view(torch.float32)


@pytest.mark.parametrize("shape", sb.SHAPES, ids=lambda s: f"rows{s[0]}-A{s[1]}")
def test_kernel_equals_the_reference_on_the_shared_cases(torch_cuda, shape):
    torch = torch_cuda
    from isaacgym_amd.sensor import SensorLine
    worst = 0.0
    for case in (c for c in CASES if (c["rows"], c["A"]) == shape):
        rows, W, ld = case["rows"], case["W"], case["ld"]
        data, ref = sb.case_data(case), sb.run_reference(case)
        kw = sb.line_kwargs(case, data)
        line = SensorLine(rows, W, DEV, **kw)
        line.held.view(torch.int32).fill_(np.uint32(sb.CANARY).astype(np.int32).item())
        table = None if case["draw"] else (line.sigma.clone(), line.drop.clone())
        xs = []
        for t in range(sb.PUSHES):
            back, flat = phased(torch, rows * ld, case["phase_in"])
            flat.copy_(torch.from_numpy(np.ascontiguousarray(data["xs"][t]).view(np.int32).reshape(-1)).to(DEV))
            xs.append((back, flat.view(rows, ld)))
        keep = [b.clone() for b, _ in xs]
        dones = torch.from_numpy(data["dones"]).to(DEV)
        out_back, out_flat = phased(torch, rows * ld, case["phase_out"])
        out = out_flat.view(rows, ld)
        for t in range(sb.PUSHES):
            where = (case["id"], t)
            line.push(f32(xs[t][1])[:, :W], dones[t], f32(out)[:, :W])
            got = out[:, :W].cpu().numpy().view(np.uint32)
            assert np.array_equal(line.age.cpu().numpy(), ref[t]["age"]) and np.array_equal(line.episode.cpu().numpy(), ref[t]["episode"]), where
            for name in ("sigma", "drop"):
                assert np.array_equal(getattr(line, name).cpu().numpy().view(np.uint32), ref[t][name].view(np.uint32)), (where, name)
            worst = max(worst, sb.compare(got, ref[t], 4 * E_MEASURED, where))
            # held after a push is what the push delivered (a dropped row delivered it, a fresh one stored it); a drop decision that differs
            # from the reference's shows in the delivered words above (test_dropped_rows_deliver_the_held_words_bit_for_bit counts them)
            held = line.held.cpu().numpy().view(np.uint32)
            hold = np.broadcast_to(data["col_hold"] != 0, held.shape)
            assert np.array_equal(held[hold], got[hold]), where
            assert (held[~hold] == sb.CANARY).all(), where                                          # held is touched only for hold columns
            if ld > W:
                assert (out[:, W:].cpu().numpy().view(np.uint32) == sb.CANARY).all(), where         # canaries past W in every row
        guard = out_back.cpu().numpy().view(np.uint32)
        assert (guard[:4 + case["phase_out"]] == sb.CANARY).all() and (guard[4 + case["phase_out"] + rows * ld:] == sb.CANARY).all(), case["id"]
        assert all(torch.equal(b, k) for (b, _), k in zip(xs, keep)), case["id"]                    # the input, padding and guards included, is not modified
        if table is not None:                                                                       # draw = 0: the kernel never writes the caller's table
            assert torch.equal(line.sigma, table[0]) and torch.equal(line.drop, table[1]), case["id"]
    print(f"device Box-Muller against fp64 over rows{shape[0]}-A{shape[1]}: worst {worst:.3e} of a unit normal (E_MEASURED {E_MEASURED:.3e}, asserted at 4 x)")


def test_dropped_rows_deliver_the_held_words_bit_for_bit(torch_cuda):
    """Every drop decision, seen from outside: with sigma = 0 a row's output is either its input (not dropped) or its previous output."""
    torch = torch_cuda
    from isaacgym_amd import sensor
    rows, W, A = 130, 27, 2
    drop = np.full(rows, 0.5, np.float32)
    line = sensor.SensorLine(rows, W, DEV, num_agents=A, sigma=np.zeros(rows, np.float32), drop=drop, seed=sb.STREAM, env_id_offset=9)
    ref = sensor.reference(rows, W, A, sigma=np.zeros(rows, np.float32), drop=drop, seed=sb.STREAM, env_id_offset=9)
    rng = np.random.default_rng(2)
    seen = 0
    for t in range(12):
        x = rng.uniform(-1, 1, (rows, W)).astype(np.float32)
        done = np.repeat((rng.random(rows // A) < 0.2).astype(np.int64), A)
        got = line.push(torch.from_numpy(x).to(DEV), torch.from_numpy(done).to(DEV)).cpu().numpy()
        want = ref.push(x, done)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
        seen += int(ref.dropped.sum())
    assert rows * 12 * 0.3 < seen < rows * 12 * 0.6


def test_a_captured_push_replays_like_eager_pushes(torch_cuda):
    """No host-side counter, the level draws and the drop decisions included: one captured push replayed equals the eager sequence."""
    torch = torch_cuda
    from isaacgym_amd.sensor import SensorLine
    rows, A, W, T = 130, 2, 27, 12
    rng = np.random.default_rng(4)
    x_dev = torch.from_numpy(rng.uniform(-2, 2, (T, rows, W)).astype(np.float32)).to(DEV)
    done_dev = torch.from_numpy(np.repeat((rng.random((T, rows // A)) < 0.2).astype(np.int64), A, axis=1)).to(DEV)
    kw = dict(num_agents=A, sigma=(0.0, 0.5), drop=(0.1, 0.6), hold_columns=(np.arange(W) >= 20), seed=sb.STREAM, env_id_offset=5, key_period=30)
    eager, replayed = (SensorLine(rows, W, DEV, **kw) for _ in range(2))
    out_e, out_r = (torch.zeros((rows, W), dtype=torch.float32, device=DEV) for _ in range(2))
    want = [(eager.push(x_dev[t], done_dev[t], out_e).clone(), eager.sigma.clone(), eager.drop.clone()) for t in range(T)]
    x, done = x_dev[0].clone(), done_dev[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        replayed.push(x, done, out_r)                                                       # warm-up outside the capture ...
        replayed.reset()                                                                    # ... undone
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.push(x, done, out_r)
    replayed.reset()                                                                        # the capture itself ran nothing
    for t in range(T):
        x.copy_(x_dev[t])
        done.copy_(done_dev[t])
        graph.replay()
        assert torch.equal(out_r.view(torch.int32), want[t][0].view(torch.int32)), t
        assert torch.equal(replayed.sigma, want[t][1]) and torch.equal(replayed.drop, want[t][2]), t
    assert torch.equal(replayed.age, eager.age) and torch.equal(replayed.episode, eager.episode)
    assert torch.equal(replayed.held.view(torch.int32), eager.held.view(torch.int32))


def test_the_noise_has_the_moments_of_a_standard_normal(torch_cuda):
    """One channel of rows = 2048, W = 80, one push, sigma = 1 on zeros: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)."""
    torch = torch_cuda
    from isaacgym_amd import scene, sensor
    rows, W = 2048, 80
    n = rows * W
    seed = scene.stream_seed(MOMENT_SEED, scene.STREAM_SENSOR)
    one, zero = np.ones(rows, np.float32), np.zeros(rows, np.float32)
    want = sensor.reference(rows, W, sigma=one, drop=zero, seed=seed).push(np.zeros((rows, W), np.float32)).astype(np.float64)
    got = sensor.SensorLine(rows, W, DEV, sigma=one, drop=zero, seed=seed).push(torch.zeros((rows, W), device=DEV), None).cpu().numpy().astype(np.float64)
    for name, g in (("reference", want), ("device", got)):
        print(f"{name}: mean {g.mean():+.3e} (bound {5 / np.sqrt(n):.3e}), var - 1 {g.var() - 1:+.3e} (bound {5 * np.sqrt(2 / n):.3e})")
        assert abs(g.mean()) <= 5 / np.sqrt(n) and abs(g.var() - 1) <= 5 * np.sqrt(2 / n), name
    assert np.abs(got - want).max() <= 4 * E_MEASURED + 2.0 ** -23 * np.abs(want).max()
    assert abs(np.corrcoef(got[:, 0::2].ravel(), got[:, 1::2].ravel())[0, 1]) <= 5 / np.sqrt(n / 2)      # the two branches of a pair


def test_the_drop_share_is_the_probability(torch_cuda):
    """rows = 2048, 20 pushes, drop = 0.3: the share of dropped samples among those that can drop (all but each episode's first) is within
    5 sqrt(p (1 - p) / n) of p.  sigma = 0, so a row's output is its input or its previous output: counted from outside."""
    torch = torch_cuda
    from isaacgym_amd import scene, sensor
    rows, W, T, p = 2048, 4, 20, 0.3
    seed = scene.stream_seed(DROP_SEED, scene.STREAM_SENSOR)
    zero, drop = np.zeros(rows, np.float32), np.full(rows, p, np.float32)
    ref, line = sensor.reference(rows, W, sigma=zero, drop=drop, seed=seed), sensor.SensorLine(rows, W, DEV, sigma=zero, drop=drop, seed=seed)
    dropped_ref = dropped_dev = 0
    for t in range(T):
        x = np.full((rows, W), float(t + 1), np.float32)
        ref.push(x)
        got = line.push(torch.from_numpy(x).to(DEV), None).cpu().numpy()
        dropped_ref += int(ref.dropped.sum())
        dropped_dev += int((got[:, 0] != t + 1).sum())
    n = rows * (T - 1)
    bound = 5 * np.sqrt(p * (1 - p) / n)
    print(f"drop share: reference {dropped_ref / n:.5f}, device {dropped_dev / n:.5f}, p {p} +- {bound:.5f}")
    assert dropped_dev == dropped_ref
    assert abs(dropped_ref / n - p) <= bound and abs(dropped_dev / n - p) <= bound


def test_sensor_line_checks_its_arguments_on_the_host(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.sensor import SensorLine
    for kw in (dict(rows=0), dict(rows=3, num_agents=2), dict(num_agents=3), dict(width=0), dict(width=513), dict(sigma=-1.0), dict(sigma=(2, 1)), dict(drop=1.5),
               dict(channel=2), dict(env_id_offset=-1), dict(key_period=-1), dict(sigma=np.zeros(4, np.float32), drop=(0.0, 0.1)), dict(columns=np.ones(2)),
               dict(columns=-np.ones(3)), dict(hold_columns=np.full(3, 2)), dict(sigma=np.full(4, -1.0), drop=np.zeros(4)), dict(sigma=np.zeros(4), drop=np.full(4, 2.0)),
               dict(sigma=np.zeros(5), drop=np.zeros(5))):
        a = dict(rows=4, width=3, device=DEV, num_agents=1, sigma=0.1, drop=0.1, seed=1)
        a.update(kw)
        with pytest.raises(ValueError, match="SensorLine"):
            SensorLine(**a)
    table = SensorLine(4, 3, DEV, sigma=np.full(4, 0.5, np.float32))                          # a per-row array beside one number: both are the caller's table
    assert table.draw == 0 and (table.drop == 0).all() and (table.sigma == 0.5).all()
    line = SensorLine(4, 3, DEV, sigma=0.1, drop=0.1)
    good, out = torch.zeros((4, 3), device=DEV), torch.zeros((4, 3), device=DEV)
    for bad in (torch.zeros((3, 4), device=DEV).t(), good.double(), good[:-1], good.cpu()):
        with pytest.raises(ValueError, match="SensorLine.push: x"):
            line.push(bad, None, out)
        with pytest.raises(ValueError, match="SensorLine.push: out"):
            line.push(good, None, bad)
    with pytest.raises(ValueError, match="SensorLine.push: done"):
        line.push(good, torch.zeros(4, dtype=torch.int32, device=DEV), out)
    assert not line.age.any()                                                                 # nothing was launched
