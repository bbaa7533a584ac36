"""Short trajectories for the step kernels' wave hand-offs (tests/test_step_hybrid_schedule_host.py / _gpu.py): 8 oracle steps per case
from a state in which the arm MOVES and the ball is on its way to it, so that the collision geometry of the later substep boundaries — the
part of a step that crosses from the arm wave to the ball wave — decides where the ball goes.

A case is (variant, num_envs, substeps, randomised).  Every env gets a drawn arm pose inside the limits, drawn joint velocities and drawn
actions around the pose's own; its ball flies at 2 - 5 m/s towards the blade centre, the hand or the forearm (env % 3) as they stand at the
start, due there after 0.2 - 6 control steps.  Gravity and the arm's motion are ignored in the aim: the balls arrive NEAR the body, some
hit, the others pass through the bounding spheres, and which did is read off the oracle (below), never assumed.

Everything here comes from the oracle and the config.  `arm_contacts` counts the env-steps in which a second oracle whose config has the
paddle and the six shapes taken away (ball_contact_scenarios.counterfactual_configs' recipe) ends with another ball velocity: the
env-steps that depend on the arm's geometry.  SEEDS holds, per case, the scenario seed: the smallest for which the oracle's own
sensitivity probe sets aside at most EXCLUDED_CAP of the case's env-steps and the arm is reached at all (tools are not needed: the host
test asserts both for every case, so a changed oracle or scenario shows there, without a GPU)."""
import functools
import types

import numpy as np

import ball_contact_scenarios as sc
from helpers import SensitivityProbe
from isaacgym_amd import scene

STEPS = 8
ENV_SEED = 5
EXCLUDED_CAP = 0.02
VARIANTS = ("TT", "TN", "T3")
SIZES = (1, 63, 65, 130)          # a lone lane, a ragged workgroup, a second workgroup with one lane, a second ragged workgroup
SUBSTEPS = (1, 2, 3, 4)           # no handed-over boundary, one, and the later hand-off slots
CASES = [(v, n, s, dr) for v in VARIANTS for n in SIZES for s in SUBSTEPS for dr in (False, True)]

# scenario seed per case where 0 does not do (see the module docstring): the plain TT / TN cases at 65 and 130 envs, whose seed-0 draws put
# more env-steps than the cap allows within the probe's reach of a contact switch
SEEDS = {(v, n, s, False): seed for v in ("TT", "TN") for n, seed in ((65, 2), (130, 1)) for s in SUBSTEPS}


def seed_of(variant, n, substeps, dr):
    return SEEDS.get((variant, n, substeps, dr), 0)


def min_arm_contacts(n):
    """Env-steps of a case that must depend on the arm's geometry: one for a lone env, n / 16 (at least 2) otherwise."""
    return 1 if n == 1 else max(2, n // 16)


def case_config(variant, n, substeps):
    cfg = scene.build_config(variant, num_envs=n, seed=ENV_SEED)
    cfg.substeps = substeps
    return cfg


def case_tables(variant, n, seed):
    return sc._tables(variant, n, np.random.default_rng([seed, 78]), np.zeros(n, bool))


def _without_arm(cfg):
    c = sc._copy(cfg)
    c.paddle_radius, c.paddle_half_thickness = 1e-9, 1e-9
    c.paddle_center[2] = 100.0
    for s in range(len(sc.SHAPES)):
        sh = c.shape[s]
        sh.radius = 1e-9
        for k in range(3):
            sh.a[k] = sh.b[k] = (0.0, 0.0, 100.0 if sh.link >= 0 else -100.0)[k]
    return c


def start_state(o, cfg, n, rng):
    """Sets the oracle `o` to the drawn start state; -> the arm pose's own actions [n, 7]."""
    u = lambda lo_, hi_, shape=n: rng.uniform(lo_, hi_, shape)
    lo, hi = (np.array([getattr(cfg.joint[j], k) for j in range(7)], np.float64) for k in ("lower", "upper"))
    q = np.clip(u(-0.6, 0.6, (7, n)), (lo + 0.01)[:, None], (hi - 0.01)[:, None])
    o.dof_pos[:], o.dof_vel[:] = q, u(-2.0, 2.0, (7, n))
    arm = sc.Arm(cfg, o.refresh_rigid_body_states().astype(np.float64), 0)
    hand_a = arm.shape(0)[0]
    fa, _, fb, _, _ = arm.shape(1)
    target = np.select([(np.arange(n) % 3 == 0)[:, None], (np.arange(n) % 3 == 1)[:, None]], [arm.pc, hand_a], fa + (fb - fa) * u(0.2, 0.8)[:, None])
    d = sc._unit(np.stack([-np.ones(n), u(-0.4, 0.4), u(-0.4, 0.4)], 1))
    v = d * u(2.0, 5.0)[:, None]
    t_hit = u(0.2, 6.0) * float(cfg.dt)
    o.ball[0:3] = (target - v * t_hit[:, None]).T
    o.ball[7:10] = v.T
    o.ball[10:13] = u(-30.0, 30.0, (3, n))
    return np.clip((q - 0.5 * (hi + lo)[:, None]) / (0.5 * (hi - lo))[:, None], -1, 1).T


@functools.lru_cache(maxsize=None)
def oracle_run(variant, n, substeps, dr, seed=None):
    """The reference trajectory of a case: STEPS oracle steps.  -> namespace(cfg, probe, tables, steps, excluded, arm_contacts); a step is a
    dict: st (the oracle's state blob at its start), act, main (snapshot of the oracle after it), keep (~ SensitivityProbe.sensitive), edge
    (zeros: ball_contact_scenarios.compare_step's plain tolerances).  Computed once per case and shared; nothing in it is to be written to."""
    from oracle import binding
    binding.build()
    seed = seed_of(variant, n, substeps, dr) if seed is None else seed
    cfg = case_config(variant, n, substeps)
    tables = case_tables(variant, n, seed) if dr else None

    def make(c):
        x = binding.OracleEnv(c, threads=4)
        if dr:
            x.set_randomization(**tables, **sc.DR_NOISE)
        return x
    o, bare = make(cfg), make(_without_arm(cfg))
    probe = SensitivityProbe(binding, cfg)
    if dr:
        probe.o2.set_randomization(**tables, **sc.DR_NOISE)
    rng = np.random.default_rng([seed, 3])
    hold = start_state(o, cfg, n, rng)
    steps, excluded, contacts = [], 0, 0
    for t in range(STEPS):
        act = np.clip(hold + rng.uniform(-0.3, 0.3, (n, 7)), -1.2, 1.2).astype(np.float32)
        st = o.get_state()
        o.step(act)
        main = sc.snapshot(o)
        bare.set_state(st)
        bare.step(act)
        contacts += int((np.abs(bare.ball[7:10] - main.ball[7:10]).max(axis=0) > 1e-3).sum())
        keep = ~probe.sensitive(st, act, o)
        excluded += int((~keep).sum())
        steps.append(dict(st=st, act=act, main=main, keep=keep, edge=np.zeros(n)))
    bare.close()
    return types.SimpleNamespace(cfg=cfg, probe=probe, tables=tables, steps=steps, excluded=excluded, arm_contacts=contacts, num_agents=1)
