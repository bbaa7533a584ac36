"""The KEYING of the device's random streams: draws that must be independent are different numbers.

Every stochastic value of the library comes from one counter function, rng_uniform(seed, gid, episode, k) (ppenv_device.h), or from the
SplitMix form of the 27-dof reset.  The parity tests compare it with an oracle that restates the same keys, and the moment tests look at
one (seed, counter): neither sees two logical draws landing on one key.  Here the keys are looked at from outside, through the host
builds of the kernels' code (tests/csrc/host_shim.cpp, dr_shim.cpp, the oracle) and a vectorised numpy restatement that is itself checked
against them, under the seeds the product's owners of a USER seed hand the native layer: the task classes (VecTask.native_seeds,
build_native_config — what create_sim and the reset-randomisation plan use) and policy.sampler_stream_seed (what PPOTrainer and
RLGamesPolicy.act use); tests/test_rng_streams_gpu.py drives the tasks, the trainer and act themselves:

  a. distinctness over the key lattice the product generates: seeds next to each other, data-parallel shards (seed + r, offset r n),
     sampler rows of eight ranks, one user seed in every family, the noise indices of one env-step;
  b. chi-square and lag-1 correlation with thresholds derived from the sample sizes (seeds are fixed: the values are deterministic and
     stand next to their thresholds);
  c. shards under one COMMON seed reproduce the single handle env for env.

A *stream* is the tuple of the first draws of one logical user (an env, a sampler row) under one key, e.g. 2 episodes x 3 draws; two
streams are the same only if the whole tuple is: for 24-bit draws that does not happen by chance.

What makes (a) hold: no kernel is keyed by a user seed as given (scene.stream_seed).  With the raw seed as the key, env g
of seed s has the stream of env g ^ s ^ s' of seed s' — test_native_layer_keyed_by_raw_seeds_shares_streams counts it: 64 of 64, 4096 of
4096."""
import ctypes as C

import numpy as np
import pytest

import dr_shim_binding as drs
import shim_binding as sb
from isaacgym_amd import policy, scene, vec_task

SEED_PAIRS = [(0, 1), (6, 7), (42, 43), (42, 49), (63, 64), (4095, 4096)]
NOISE_SALT = 0x5DEECE66D                      # dr_gauss_pair's own, in the kernel
U32, U64 = np.uint32, np.uint64
_cfgs = {}


def host():
    L = sb.lib()
    u32, u64 = C.c_uint32, C.c_uint64
    L.shim_rng_uniform.restype = L.shim_dr_gauss.restype = C.c_float
    L.shim_rng_uniform.argtypes = [u64, u32, u32, u32]
    L.shim_dr_gauss.argtypes = [u64, u32, u32, u32, u32]
    return L


TASKS = {"T3": vec_task.HumanoidPingpong, "TT": vec_task.HumanoidPingpongTilt, "TN": vec_task.HumanoidPingpongTiltNoEarlyStop, "T4": vec_task.Humanoid12PingpongTilt}


def config(variant, seed, env_id_offset=0, num_envs=64):
    """the ppenv_config the task class builds in create_sim for a task cfg with the USER seed `seed`"""
    key = (variant, seed, env_id_offset, num_envs)
    if key not in _cfgs:
        cfg = scene.default_task_cfg(variant)
        cfg["seed"], cfg["env_id_offset"] = seed, env_id_offset
        _cfgs[key] = TASKS[variant].build_native_config(cfg, num_envs)
    return _cfgs[key]


# ---- the seed each family's kernels are keyed by for a user seed: what the owners of the user seed derive
def env_seed(seed):
    return vec_task.VecTask.native_seeds({"seed": seed})[0]


ta_seed = env_seed          # the 27-dof task hands the same one to TAEnv: its reset draws and its noise


def tables_seed(seed):
    return vec_task.VecTask.native_seeds({"seed": seed})[1]


sampler_seed = policy.sampler_stream_seed


# ---- numpy restatement of ppenv_device.h (checked against the host build in the first test)
def hash32(x):
    x = np.atleast_1d(np.asarray(x, U32))          # (arrays wrap silently; numpy warns on scalar overflow)
    x = (x ^ (x >> U32(16))) * U32(0x7FEB352D)
    x = (x ^ (x >> U32(15))) * U32(0x846CA68B)
    return x ^ (x >> U32(16))


def ubits(kseed, gid, episode, k):
    """rng_uniform's 24-bit integer (the float is this x 2^-24), broadcast over arrays of gid / episode / k; kseed: a python int or uint64 array."""
    scalar = all(np.ndim(x) == 0 for x in (kseed, gid, episode, k))
    ks, gid, episode, k = np.atleast_1d(np.asarray(kseed, U64)), np.atleast_1d(np.asarray(gid, U32)), np.atleast_1d(np.asarray(episode, U32)), np.atleast_1d(np.asarray(k, U32))
    lo, hi = (ks & U64(0xFFFFFFFF)).astype(U32), (ks >> U64(32)).astype(U32)
    h = hash32(gid ^ lo)
    h = hash32(h + episode * U32(0x9E3779B9) + hi)
    h = hash32(h + (k + U32(1)) * U32(0x85EBCA6B))
    return (h >> U32(8))[0] if scalar else h >> U32(8)


def mix64(z):
    z = np.atleast_1d(np.asarray(z, U64))
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def ta_ubits(kseed, gid, episode, k):
    """The 27-dof reset's draw k < 5 (ppenv_ta_task.h): mix64(mix64(seed + C (gid + 1)) + C (8 ep + k + 1)) >> 40."""
    scalar = all(np.ndim(x) == 0 for x in (kseed, gid, episode, k))
    g, one = np.array([0x9E3779B97F4A7C15], U64), U64(1)
    kseed, gid, episode, k = (np.atleast_1d(np.asarray(x, U64)) for x in (kseed, gid, episode, k))
    s = mix64(kseed + g * (gid + one))
    out = (mix64(s + g * (episode * U64(8) + k + one)) >> U64(40)).astype(U32)
    return out[0] if scalar else out


def noise_keys(progress, index, ta=False):
    """dr_gauss(.., progress, index) -> (the two rng_uniform keys of its Box-Muller pair, its branch: 0 cosine, 1 sine); ta: ta_dr_gauss's
    folding of a 512-wide index space into two 256-wide pages per step."""
    if ta:
        progress, index = 2 * progress + (index >> 8), index & 255
    k = progress * 256 + 2 * (index >> 1)
    assert np.all(2 * k + 1 < 2 ** 32)
    return 2 * k, 2 * k + 1, index & 1


def gauss64(kseed, gid, episode, progress, index, ta=False, draw_ids=False):
    """fp64 Box-Muller on the restated uniforms of dr_gauss's key; scalars or arrays that broadcast.  draw_ids: also the identity of each draw,
    (u1 bits, u2 bits, branch) packed into 49 bits — two draws are the same number exactly when these are equal."""
    k1, k2, branch = noise_keys(np.asarray(progress, np.int64), np.asarray(index, np.int64), ta)
    b1, b2 = ubits(kseed ^ NOISE_SALT, gid, episode, k1), ubits(kseed ^ NOISE_SALT, gid, episode, k2)
    u1, u2 = np.maximum(b1, 1) * 2.0 ** -24, b2 * 2.0 ** -24                     # u1 = 0 -> 2^-24, the kernel's clamp
    rad = np.sqrt(-2.0 * np.log(u1))
    g = np.where(branch == 1, rad * np.sin(2 * np.pi * u2), rad * np.cos(2 * np.pi * u2))
    if draw_ids:
        return g, (np.asarray(b1, U64) << U64(25)) | (np.asarray(b2, U64) << U64(1)) | np.asarray(branch, U64)
    return g


NOISE_INDICES = {"TT": list(range(7)) + list(range(16, 96)), "T4": list(range(14)) + list(range(16, 176)), "TA": list(range(27)) + list(range(32, 345))}


def rows_of(a):
    """[m, d] array -> the set of its rows"""
    a = np.ascontiguousarray(a)
    return set(a.view(np.dtype((np.void, a.dtype.itemsize * a.shape[1]))).ravel().tolist())


def shared(a, b):
    """number of rows of `a` that are a row of `b`; the rows of each must be distinct among themselves"""
    sa, sb_ = rows_of(a), rows_of(b)
    assert len(sa) == len(a) and len(sb_) == len(b), "streams of one seed collide"
    return len(sa & sb_)


# --------------------------------------------------------------------------------------------------- 0. the restatement is the host build
def test_restatement_is_the_host_build(oracle_lib):
    L, D = host(), drs.lib()
    rng = np.random.default_rng(0)
    for kseed, gid, ep, k in zip(rng.integers(0, 2 ** 64, 200, dtype=U64), rng.integers(0, 2 ** 32, 200), rng.integers(0, 2 ** 32, 200), rng.integers(0, 2 ** 32, 200)):
        kseed, gid, ep, k = int(kseed), int(gid), int(ep), int(k)
        assert L.shim_rng_uniform(kseed, gid, ep, k) == float(ubits(kseed, gid, ep, k)) * 2.0 ** -24
        assert D.dr_shim_uniform(kseed, gid, ep, k) == float(ubits(kseed ^ scene.DR_SEED_SALT, gid, ep, k)) * 2.0 ** -24
    for seed in (0, 1, 42, 4095, 2 ** 40 + 5, 2 ** 64 - 1):
        for salt in (scene.STREAM_ENV, scene.STREAM_TABLES, scene.STREAM_SAMPLER):
            assert scene.stream_seed(seed, salt) == int(mix64(np.array([seed ^ salt], U64))[0])
        assert len({seed, env_seed(seed), tables_seed(seed), sampler_seed(seed)}) == 4
        assert int(config("T4", seed, 64, 64).seed) == env_seed(seed) and config("T4", seed, 64, 64).env_id_offset == 64
    # dr_gauss: key pairs, branches, and libm against fp64 (fp32 libm: ~1e-6 at the radius's largest, 5.8)
    ks = env_seed(42)
    for variant in ("TT", "T4"):
        for progress in (0, 7, 159):
            for index in NOISE_INDICES[variant]:
                assert abs(L.shim_dr_gauss(ks, 9, 3, progress, index) - gauss64(ks, 9, 3, progress, index)) <= 2e-6, (progress, index)
    # the 27-dof task's folding, through the oracle's observation noise (index 32 + k)
    obs = np.zeros((4, scene.TA_NUM_OBS), np.float32)
    ep0, prog0 = np.array([0, 1, 2, 3], np.uint32), np.array([0, 1, 79, 159], np.int64)
    oracle_lib.ta_add_obs_noise(obs, 1.0, ks, ep0, prog0, env_id_offset=100)
    for e in range(4):
        for k in range(scene.TA_NUM_OBS):
            assert abs(obs[e, k] - gauss64(ks, 100 + e, int(ep0[e]), int(prog0[e]), 32 + k, ta=True)) <= 2e-6, (e, k)
    # the 27-dof reset draws: the library's own host restatement (what lays out the state at creation)
    p = scene.build_ta_params(64, seed=ta_seed(42), env_id_offset=5)
    d = scene.ta_reset_draws(p, [0, 3], [0, 7]).numpy()
    for row, (i, ep) in enumerate([(0, 0), (3, 7)]):
        u0 = np.float32(ta_ubits(ta_seed(42), 5 + i, ep, 0)) * np.float32(2.0 ** -24)
        assert d[row, 0] == np.float32(p.ball_y_lo) + np.float32(p.ball_y_hi - p.ball_y_lo) * u0


ZERO_U1_KEY = (9368744190824693952, 3742455, 0, 2, 0)     # (kernel seed, env id, episode, progress, index): a draw with u1 = 0


def test_u1_zero_clamp_gives_the_largest_finite_radius():
    """u1 = 0 (one 24-bit draw in 2^24) is clamped to 2^-24: radius sqrt(-2 ln 2^-24) = 5.768, never inf.  The key below is such a draw (found by
    searching the restatement); the host build is called on it directly."""
    L = host()
    kseed, gid, ep, progress, index = ZERO_U1_KEY
    assert kseed == env_seed(1)                              # env 3742455 of a task made with seed 1 draws it at its third step
    k1, k2, _ = noise_keys(progress, index)
    assert int(ubits(kseed ^ NOISE_SALT, gid, ep, k1)) == 0
    u2 = float(ubits(kseed ^ NOISE_SALT, gid, ep, k2)) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(2.0 ** -24))
    c, s = L.shim_dr_gauss(kseed, gid, ep, progress, index), L.shim_dr_gauss(kseed, gid, ep, progress, index + 1)
    assert np.isfinite(c) and np.isfinite(s)
    assert abs(c - rad * np.cos(2 * np.pi * u2)) <= 4e-6 and abs(s - rad * np.sin(2 * np.pi * u2)) <= 4e-6
    assert abs(np.hypot(c, s) - rad) <= 4e-6




# --------------------------------------------------------------------------------------------------- a. distinctness
def _serve_streams(variant):
    def f(seed, gids):
        return np.array([np.concatenate([sb.serve_velocity(config(variant, seed), int(g), ep) for ep in (0, 1)]) for g in gids], np.float32)
    return f


def _ta_reset_streams(seed, gids):
    p = scene.build_ta_params(64, seed=ta_seed(seed))
    ids = [int(g) for g in gids]
    return np.concatenate([scene.ta_reset_draws(p, ids, [ep] * len(ids)).numpy() for ep in (0, 1)], axis=1)


def _noise_streams(seed, gids):
    L, ks = host(), env_seed(seed)
    return np.array([[L.shim_dr_gauss(ks, int(g), ep, 0, i) for ep in (0, 1) for i in (0, 1, 2)] for g in gids], np.float32)


def _table_streams(distribution):
    def f(seed, gids):
        D, ks = drs.lib(), tables_seed(seed)
        return np.array([[D.dr_shim_base(ks, int(g), draw, k, distribution) for draw in (0, 1) for k in (0, 1, 2)] for g in gids], np.float32)
    return f


def _sampler_streams(seed, rows):
    L, ks = host(), sampler_seed(seed)
    return np.array([[L.shim_dr_gauss(ks, int(r), 0, counter, j) for counter in (1, 2) for j in (0, 1, 2)] for r in rows], np.float32)


FAMILIES = {"serve TT": _serve_streams("TT"), "serve TN": _serve_streams("TN"), "serve T3": _serve_streams("T3"), "serve T4": _serve_streams("T4"),
            "27-dof reset": _ta_reset_streams, "step noise": _noise_streams, "tables uniform": _table_streams(scene.DR_DISTRIBUTIONS["uniform"]),
            "tables gaussian": _table_streams(scene.DR_DISTRIBUTIONS["gaussian"]), "sampler": _sampler_streams}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_streams_of_neighbouring_seeds_are_distinct(family):
    """All (seed, gid < 64) streams of a family pairwise distinct, for seeds that differ in the last bit, in a few bits, and by a carry into
    bit 6 / bit 12.  Under raw seeds every pair but the 27-dof reset's shared 64 of 64."""
    f, gids, cache = FAMILIES[family], np.arange(64), {}
    for a, b in SEED_PAIRS:
        for s in (a, b):
            if s not in cache:
                cache[s] = f(s, gids)
        assert shared(cache[a], cache[b]) == 0, (family, a, b)


def test_native_layer_keyed_by_raw_seeds_shares_streams():
    """Why the owners above must derive stream seeds: the native seeds key the RNG as given (include/ppenv.h), and handed the user's seeds
    themselves they give what the tasks gave before stream_seed — neighbouring seeds share 64 of 64 env and table streams, ranks (63, offset 0) /
    (64, offset 64) 64 of 64 and (4095, 0) / (4096, 4096) 4096 of 4096, the sampler rows of ranks 42..49 are 64 streams of 512, and every
    sampler pair is an env-noise pair.  Through the host build where it takes a seed."""
    ep, k = np.repeat([0, 1], 3)[None, :], np.tile([0, 1, 2], 2)[None, :]
    g = np.arange(64)
    for a, b in [(0, 1), (6, 7), (42, 43), (42, 49)]:
        assert shared(_env_lattice(a, g), _env_lattice(b, g)) == 64
        assert shared(ubits(a ^ scene.DR_SEED_SALT, g.astype(U32)[:, None], ep, k), ubits(b ^ scene.DR_SEED_SALT, g.astype(U32)[:, None], ep, k)) == 64
        assert shared(ta_ubits(a, g[:, None], ep, k), ta_ubits(b, g[:, None], ep, k)) == 0          # the SplitMix form never had it
    for n, s in [(64, 63), (4096, 4095)]:
        assert shared(_env_lattice(s, np.arange(n)), _env_lattice(s + 1, n + np.arange(n))) == n
    L = host()
    raw = lambda seed, rows: np.array([[L.shim_dr_gauss(seed, int(r), 0, c, j) for c in (1, 2) for j in (0, 1, 2)] for r in rows], np.float32)
    assert len(rows_of(np.concatenate([raw(42 + r, g) for r in range(8)]))) == 64
    smp = _pairs(42 ^ NOISE_SALT, g, [0], [c * 256 + 2 * j for c in range(8) for j in range(14)])
    noi = _pairs(42 ^ NOISE_SALT, g, [0, 1], [p * 256 + 2 * j for p in range(8) for j in range(48)])
    assert np.intersect1d(smp, noi).size == smp.size == 7168


def _env_lattice(kseed, gids):
    """uniform-level streams of the three rng_uniform users of one env seed: serve keys, noise keys (under the noise salt) — [n, 12] 24-bit ints"""
    g = np.asarray(gids, U32)[:, None]
    ep, k = np.repeat([0, 1], 3)[None, :], np.tile([0, 1, 2], 2)[None, :]
    return np.concatenate([ubits(kseed, g, ep, k), ubits(kseed ^ NOISE_SALT, g, ep, k)], axis=1)


@pytest.mark.parametrize("n,seed", [(64, 42), (64, 63), (4096, 4095)])
def test_data_parallel_shards_share_no_stream(n, seed):
    """Shards as the ranks of a data-parallel run build them: rank r has seed + r and env_id_offset r n.  Under raw seeds (63, 64) at n = 64 shared
    64 of 64 env streams and (4095, 4096) at n = 4096 shared 4096 of 4096: the carry of seed + 1 reaches the offset bit."""
    g0, g1 = np.arange(n), n + np.arange(n)
    assert shared(_env_lattice(env_seed(seed), g0), _env_lattice(env_seed(seed + 1), g1)) == 0
    ep, k = np.repeat([0, 1], 3)[None, :], np.tile([0, 1, 2], 2)[None, :]
    assert shared(ta_ubits(ta_seed(seed), g0[:, None], ep, k), ta_ubits(ta_seed(seed + 1), g1[:, None], ep, k)) == 0
    t0, t1 = tables_seed(seed) ^ scene.DR_SEED_SALT, tables_seed(seed + 1) ^ scene.DR_SEED_SALT
    assert shared(ubits(t0, g0.astype(U32)[:, None], ep, k), ubits(t1, g1.astype(U32)[:, None], ep, k)) == 0
    if n == 64:                                    # ... and through the host build itself
        for name in ("serve TT", "serve T4", "27-dof reset", "step noise", "tables uniform", "tables gaussian"):
            assert shared(FAMILIES[name](seed, g0), FAMILIES[name](seed + 1, g1)) == 0, name


def test_sampler_rows_of_eight_ranks_are_512_streams():
    """The trainer's CLI gives rank r seed + r, and the sampler keys by the LOCAL row: under raw seeds 42..49 all eight ranks drew the same
    exploration noise, permuted within blocks of 32 rows (64 distinct streams of 512)."""
    s = np.concatenate([_sampler_streams(42 + r, np.arange(64)) for r in range(8)])
    assert len(rows_of(s)) == 512


def _pairs(kseed, gid, episode, pair):
    """the 48-bit Box-Muller / serve draw pairs (u(2 pair), u(2 pair + 1)) over the outer product of the three axes, flattened"""
    g, e, p = np.meshgrid(np.asarray(gid, U32), np.asarray(episode, U32), np.asarray(pair, U32), indexing="ij")
    return (ubits(kseed, g, e, 2 * p).astype(U64) << U64(24) | ubits(kseed, g, e, 2 * p + U32(1)).astype(U64)).ravel()


@pytest.mark.parametrize("seed", [0, 42, 4095])
def test_families_under_one_user_seed_share_no_draw(seed):
    """The CLI hands ONE seed to the task, its randomisation plan and the trainer.  Every family's draws are pairs (u(2 j), u(2 j + 1)) of the
    counter RNG — the serve's (speed, tilt), a Box-Muller pair — so a shared key shows as a shared 48-bit pair; by chance, 2e5 pairs share one
    with probability 1e-4.  Under raw seeds the sampler's pair (row, counter, j) WAS the env noise's (gid = row, episode 0, progress = counter, j):
    every one of the sampler's 64 x 8 x 14 pairs below was also an env's."""
    gid = np.arange(64)
    sets = {"serve": _pairs(env_seed(seed), gid, [0, 1], [0, 1]),
            "noise": _pairs(env_seed(seed) ^ NOISE_SALT, gid, [0, 1], [p * 256 + 2 * j for p in range(8) for j in range(48)]),   # TT's 96 indices, progress 0..7
            "tables": _pairs(tables_seed(seed) ^ scene.DR_SEED_SALT, gid, [0, 1], np.arange(5 * scene.DR_MAX_ROWS // 2)),
            "sampler": _pairs(sampler_seed(seed) ^ NOISE_SALT, gid, [0], [c * 256 + 2 * j for c in range(8) for j in range(14)])}  # counter 0..7, 27 actions
    names = list(sets)
    for i, a in enumerate(names):
        assert len(np.unique(sets[a])) == sets[a].size, a
        for b in names[i + 1:]:
            assert np.intersect1d(sets[a], sets[b]).size == 0, (a, b)
    # the sampler against the env's noise through the host build: (row, counter) v (gid, episode, progress), same index
    L, se, ss = host(), env_seed(seed), sampler_seed(seed)
    env = {L.shim_dr_gauss(se, g, ep, p, j) for g in range(16) for ep in (0, 1) for p in range(8) for j in range(7)}
    smp = {L.shim_dr_gauss(ss, r, 0, c, j) for r in range(16) for c in range(8) for j in range(7)}
    assert len(env) == 16 * 2 * 8 * 7 and len(smp) == 16 * 8 * 7 and not (env & smp)


@pytest.mark.parametrize("task", ["TT", "T4", "TA"])
def test_noise_indices_of_one_env_step_have_their_own_keys(task):
    """Within one env-step every noise index draws from its own (uniform key pair, branch), and none is a key of the next step's: TT actions 0-6
    and observations 16-95, T4 0-13 and 16-175, TA 0-26 and 32-344 through ta_dr_gauss's two pages.  (noise_keys is checked against the host
    build and the oracle above.)"""
    idx = NOISE_INDICES[task]
    for progress in (0, 1, 158):
        keys = [noise_keys(p, i, task == "TA") for p in (progress, progress + 1) for i in idx]
        assert len(set(keys)) == 2 * len(idx)
        pairs = {(k1, k2) for k1, k2, _ in keys}
        assert len(pairs) == 2 * {"TT": 4 + 40, "T4": 7 + 80, "TA": 14 + 112 + 45}[task]        # indices 2 j and 2 j + 1 share a pair, by design
        flat = [k for k1, k2, _ in keys for k in (k1, k2)]
        assert len(set(flat)) == 2 * len(pairs)                      # no uniform serves two pairs
    if task != "TA":                                                  # the values, through the host build
        L, ks = host(), env_seed(5)
        vals = [L.shim_dr_gauss(ks, 3, 1, p, i) for p in (4, 5) for i in idx]
        assert len(set(vals)) == len(vals)


# --------------------------------------------------------------------------------------------------- b. regression guards
CHI2_BOUND = 63 + 6 * np.sqrt(126.0)          # 64 bins: mean 63, sd sqrt(126); 130.35


def _chi2(bits):
    assert bits.size == 2 ** 18
    c = np.bincount((bits.ravel() >> U32(18)).astype(np.int64), minlength=64).astype(np.float64)
    return float(((c - 4096.0) ** 2 / 4096.0).sum())


def _family_draws():
    g12, g10, g8, g6 = (np.arange(1 << b, dtype=U32) for b in (12, 10, 8, 6))
    m = lambda *ax: np.meshgrid(*ax, indexing="ij")
    g, e, k = m(g12, np.arange(16), np.arange(4))
    yield "serve", ubits(env_seed(7), g, e, k)                                       # 4096 envs x 16 episodes x 4 keys
    yield "27-dof reset", ta_ubits(ta_seed(7), g, e, k)
    noise_k = lambda steps, pairs: (np.arange(steps)[:, None, None] * 512 + np.arange(pairs)[None, :, None] * 4 + np.arange(2)[None, None, :]).ravel()
    g, e, k = m(g6, np.arange(2), noise_k(8, 128))
    yield "step noise", ubits(env_seed(7) ^ NOISE_SALT, g, e, k)                     # 64 envs x 2 episodes x 8 steps x 128 pairs x 2
    g, e, k = m(g10, np.arange(4), np.arange(64))
    yield "tables", ubits(tables_seed(7) ^ scene.DR_SEED_SALT, g, e, k)              # 1024 envs x 4 redraws x 64 keys
    g, e, k = m(g8, np.arange(1), noise_k(8, 64))
    yield "sampler", ubits(sampler_seed(7) ^ NOISE_SALT, g, e, k)                    # 256 rows x 8 counters x 64 pairs x 2


def test_chi_square_of_every_family():
    """64 bins of 2^18 draws per family under user seed 7: chi-square < 63 + 6 sqrt(126) = 130.3 (six sigma of the 63-dof distribution).
    Measured on the host build: serve 69.0, 27-dof reset 50.1, step noise 59.9, tables 60.6, sampler 73.4."""
    for name, bits in _family_draws():
        x = _chi2(bits)
        print(f"chi-square [{name}] = {x:.1f}")
        assert x < CHI2_BOUND, (name, x)


def _lag1(bits):
    """correlation of consecutive draws along the LAST axis, pooled over the others -> (r, n pairs)"""
    u = bits.astype(np.float64) * 2.0 ** -24 - 0.5
    a, b = u[..., :-1].ravel(), u[..., 1:].ravel()
    return float(np.corrcoef(a, b)[0, 1]), a.size


def _lag1_cases():
    n = np.arange(16385, dtype=U32)
    four = np.arange(4, dtype=U32)[:, None]
    ks, kn, kt = env_seed(7), env_seed(7) ^ NOISE_SALT, ta_seed(7)
    yield "gid", ubits(ks, n[None, :], four, 1)                                      # 4 episodes x 16384 pairs of neighbouring envs
    yield "episode", ubits(ks, four, n[None, :], 1)
    yield "k", ubits(ks, four, 0, n[None, :])
    yield "progress", ubits(kn, four, 0, n[None, :].astype(U32) * U32(512))          # the first uniform of noise index 0, step by step
    seeds = mix64((np.arange(16385, dtype=U64) ^ U64(scene.STREAM_ENV)))
    assert int(seeds[7]) == ks
    yield "seed", ubits(seeds[None, :], four, 0, 0)                                  # user seeds 0 .. 16384 at 4 envs
    yield "27-dof gid", ta_ubits(kt, n[None, :], four, 1)
    yield "27-dof episode", ta_ubits(kt, four, n[None, :], 1)
    yield "27-dof seed", ta_ubits(seeds[None, :], four, 0, 0)


def test_lag_one_correlation_along_every_key_axis():
    """Neighbours along one key axis at a time — env id, episode, draw, progress, user seed: |r| <= 6 / sqrt(n) for the n = 65536 pairs (0.0234).
    Measured on the host build: gid -0.00347, episode +0.00663, k +0.00110, progress +0.00073, seed -0.00017; the 27-dof reset's SplitMix form:
    gid -0.00145, episode -0.00167, seed +0.00006."""
    for name, bits in _lag1_cases():
        r, n = _lag1(bits)
        print(f"lag-1 [{name}] r = {r:+.5f} (n = {n})")
        assert n == 65536 and abs(r) <= 6.0 / np.sqrt(n), (name, r)


# --------------------------------------------------------------------------------------------------- c. the invariant that must survive
def test_shards_under_a_common_seed_are_the_single_handle():
    """(seed, env_id_offset = r n, local env e) is env r n + e of the single handle, stream for stream: the stream seed is a function of the user
    seed alone, and the global env id is the key.  (Device level: tests/test_gpu_parity.py, test_distributed_gloo.py.)"""
    n, seed = 64, 42
    for variant in ("TT", "T4"):
        for e in (0, 1, 63):
            a = [sb.serve_velocity(config(variant, seed, n, n), n + e, ep) for ep in (0, 1)]
            b = [sb.serve_velocity(config(variant, seed, 0, 2 * n), n + e, ep) for ep in (0, 1)]
            np.testing.assert_array_equal(a, b)
    ids = list(range(n))
    for ep in (0, 1):
        shard = scene.ta_reset_draws(scene.build_ta_params(n, seed=ta_seed(seed), env_id_offset=n), ids, [ep] * n).numpy()
        whole = scene.ta_reset_draws(scene.build_ta_params(2 * n, seed=ta_seed(seed)), [n + i for i in ids], [ep] * n).numpy()
        np.testing.assert_array_equal(shard, whole)
    plan = drs.mixed_plan(frequency=1)
    shard, whole = drs.HostDR(plan, n, seed=tables_seed(seed), env_id_offset=n), drs.HostDR(plan, 2 * n, seed=tables_seed(seed))
    for _ in range(2):
        shard.apply(np.ones(n, np.int64)); whole.apply(np.ones(2 * n, np.int64))
    for name in shard.tables:
        np.testing.assert_array_equal(whole.tables[name][:, n:].view(np.uint32), shard.tables[name].view(np.uint32))
