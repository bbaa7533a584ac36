"""Per-env domain randomisation of an environment handle, and `NativeEnv`: the surface every task's env has (PPEnv, TAEnv), stated once.
`Randomizable` is the surface PPEnv and TASim share: the tables a caller hands over, the noise amplitudes, and the reset-time plan.  `ResetRandomizer` is reset-time randomisation drawn on the device
(include/ppenv_dr.h): the tables, the uploaded plan and the state block of one environment handle, and the two launches.  The reference's rule — an env's actor parameters are redrawn when THAT env
resets (tasks/humanoid_pingpong_3_actor_tilt.py:849-850, 1025; upstream VecTask.apply_randomizations) — without a host round trip.
torch owns the memory, as it owns the environments' arenas; the library rewrites table columns in place."""
import ctypes as C

import torch

from . import _lib, scene

# the per-env tables of set_randomization, in the order of scene.Randomization's pointers (the keys of every DR_TABLE_ROWS)
TABLE_NAMES = ("dof_stiffness_scale", "dof_damping_scale", "link_mass_scale", "restitution_scale", "friction_scale")


class ResetRandomizer:
    def __init__(self, L, device, num_envs, plan, table_rows, seed=0, env_id_offset=0, reset_rows=1):
        """plan: scene.reset_randomization_plan's dict.  table_rows: {set_randomization name: rows of that table for this environment,
        0 for a per-env scalar [N]}; a plan whose row counts differ was built for another task and is refused."""
        self.L, self.device, self.num_envs, self.plan = L, torch.device(device), int(num_envs), plan
        self.frequency, self.reset_rows = int(plan["frequency"]), int(reset_rows)
        n = self.num_envs
        self.tables = {}
        for name, t in plan["tables"].items():
            if name not in table_rows:
                raise ValueError(f"reset randomisation plan: this environment has no table {name!r}")
            rows = table_rows[name]
            if int(t["rows"]) != max(rows, 1):
                raise ValueError(f"reset randomisation plan: table {name!r} has {t['rows']} rows in the plan, {max(rows, 1)} in this environment")
            fill = 1.0 if t["operation"] == "scaling" else 0.0        # the neutral element: what the table holds before its env's first redraw
            self.tables[name] = torch.full((rows, n) if rows else (n,), fill, dtype=torch.float32, device=self.device)
        host = scene.build_dr_plan(plan, {k: v.data_ptr() for k, v in self.tables.items()}, n, env_id_offset=env_id_offset, seed=seed,
                                   reset_rows=reset_rows)
        self.plan_dev = torch.zeros(C.sizeof(scene.DRPlan), dtype=torch.uint8, device=self.device)
        off, nbytes = L.ppenv_dr_state_draws_offset(n), L.ppenv_dr_state_bytes(n)
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)       # all zeros = no step counted yet: the first apply redraws every env
        self.steps = self.state[:off].view(torch.int64)                               # one copy of the control-step count per workgroup, all equal
        self.draws = self.state[off:].view(torch.int32)                               # [N] redraws each env has had
        self.randomize_buf = torch.zeros(n, dtype=torch.int64, device=self.device)    # the reference's attribute: control steps since the env's last redraw
        with torch.cuda.device(self.device):
            _lib.check(L.ppenv_dr_plan_upload(C.byref(host), self.plan_dev.data_ptr(), _lib.stream(self.device)), L)

    def apply(self, reset_buf):
        """One control step of the rule (ppenv_dr_apply), after the step that wrote reset_buf [reset_rows * N] int64.  One launch, no
        synchronisation."""
        assert reset_buf.dtype == torch.int64 and reset_buf.is_contiguous() and reset_buf.numel() == self.reset_rows * self.num_envs
        _lib.check(self.L.ppenv_dr_apply(self.plan_dev.data_ptr(), self.num_envs, reset_buf.data_ptr(), self.randomize_buf.data_ptr(),
                                         self.state.data_ptr(), _lib.stream(self.device)), self.L)

    def step(self, t, rew_t, reset_t):
        """The collector's per-step hook (RolloutCollector(randomizer=)): apply(reset_t) on the row of dones the env step just wrote."""
        self.apply(reset_t)

    def apply_ids(self, env_ids):
        """The rule for the envs reset_idx(env_ids) lists (ppenv_dr_apply_ids); duplicates are dropped here (the kernel wants distinct ids)."""
        ids = torch.unique(torch.as_tensor(env_ids, dtype=torch.int64).reshape(-1).to(self.device))
        if ids.numel() == 0:
            return
        _lib.check(self.L.ppenv_dr_apply_ids(self.plan_dev.data_ptr(), self.num_envs, ids.data_ptr(), ids.numel(), self.randomize_buf.data_ptr(),
                                             self.state.data_ptr(), _lib.stream(self.device)), self.L)
        ids.record_stream(torch.cuda.current_stream(self.device))


class Randomizable:
    """The randomisation surface of a native handle (PPEnv, TASim), which has `L`, `h`, `device` and `num_envs`.  The host class
    supplies what differs: DR_TABLE_ROWS, DR_SETTER, the seed / env-id offset / reset_rows its set_reset_randomization passes on, and
    the `reset_buf` apply_reset_randomization reads."""
    DR_TABLE_ROWS = None      # {set_randomization name: rows of that table, 0 for a per-env scalar [N]}, in the order of scene.Randomization's pointers
    DR_SETTER = None          # the C setter: "ppenv_set_randomization" / "ppenv_ta_sim_set_randomization"
    _dr = None                # set_randomization's tables, kept alive here

    @property
    def dr_tables(self):
        """The tables the step reads now, in the order of DR_TABLE_ROWS (None: that one is not randomised), or None with no randomisation
        set.  Read-only: set_randomization replaces them."""
        return self._dr

    def set_randomization(self, dof_stiffness_scale=None, dof_damping_scale=None, link_mass_scale=None, restitution_scale=None,
                          friction_scale=None, action_noise_sigma=0.0, observation_noise_sigma=0.0):
        """Per-env domain-randomisation tables as float32 device tensors, [DR_TABLE_ROWS[name], N] or [N] (None = not randomised), and
        the two noise amplitudes.  The tensors are kept alive here and read by every following step; rewriting them in place changes
        the randomisation."""
        def tab(t, rows):
            if t is None:
                return None
            t = torch.as_tensor(t, dtype=torch.float32).to(self.device).contiguous()
            assert tuple(t.shape) == ((rows, self.num_envs) if rows else (self.num_envs,)), tuple(t.shape)
            return t
        given = (dof_stiffness_scale, dof_damping_scale, link_mass_scale, restitution_scale, friction_scale)
        self._dr = [tab(t, rows) for t, rows in zip(given, self.DR_TABLE_ROWS.values())]
        r = scene.Randomization()      # ppenv_ta_randomization has the fields of ppenv_randomization
        for name, t in zip(self.DR_TABLE_ROWS, self._dr):
            setattr(r, name, _lib.ptr(t))
        r.action_noise_sigma, r.observation_noise_sigma = float(action_noise_sigma), float(observation_noise_sigma)
        _lib.check(getattr(self.L, self.DR_SETTER)(self.h, C.byref(r)), self.L)

    def _set_reset_randomization(self, plan, seed, env_id_offset, reset_rows, action_noise_sigma, observation_noise_sigma):
        """What the host's set_reset_randomization does once it has filled in its defaults: the plan's tables are allocated — 1 for a
        scaling, 0 for an additive term until an env's first redraw — and handed to set_randomization with the two noise amplitudes.
        -> the ResetRandomizer (tables, randomize_buf, draws), also kept as `reset_randomization`."""
        rr = ResetRandomizer(self.L, self.device, self.num_envs, plan, self.DR_TABLE_ROWS, seed=seed, env_id_offset=env_id_offset, reset_rows=reset_rows)
        self.set_randomization(**rr.tables, action_noise_sigma=action_noise_sigma, observation_noise_sigma=observation_noise_sigma)
        self.reset_randomization = rr
        return rr

    def set_noise_sigmas(self, action_noise_sigma=0.0, observation_noise_sigma=0.0):
        """The two noise amplitudes alone, over the tables of set_reset_randomization (they stay the same tensors)."""
        self.set_randomization(**self.reset_randomization.tables, action_noise_sigma=action_noise_sigma, observation_noise_sigma=observation_noise_sigma)

    def apply_reset_randomization(self, env_ids=None):
        """The per-step launch (ppenv_dr_apply on the host's reset_buf); env_ids: the id variant, for reset_idx(env_ids)."""
        rr = getattr(self, "reset_randomization", None)
        if rr is None:
            raise _lib.PPEnvError("apply_reset_randomization: no plan is set (set_reset_randomization)")
        if env_ids is None:
            rr.apply(self.reset_buf)
        else:
            rr.apply_ids(env_ids)

    def clear_randomization(self):
        _lib.check(getattr(self.L, self.DR_SETTER)(self.h, None), self.L)
        self._dr = None
        self.reset_randomization = None


class NativeEnv:
    """What every `task.env` is — PPEnv (the three 7-dof tasks, the 4-actor task) and TAEnv (the 27-dof task) — to the code above it
    (VecTask, Player, PPOTrainer, RolloutCollector, the renderer).  The tasks differ below this surface, not in it:

    L, device                       the bound library, the torch device
    num_envs, num_agents, num_rows  num_rows = num_envs * num_agents: the rows of obs_buf / rew_buf / reset_buf / progress_buf
    num_dofs                        joints per env (7 * num_agents; 27)
    obs_buf, rew_buf, reset_buf, progress_buf
    episode, flags                  the per-env episode counter and flag words the step writes (the tensors themselves, no copy)
    status                          the device status word, 0 = healthy; read without synchronising
    DR_TABLE_ROWS, dr_tables        table name -> rows, and the tables set now (dr.Randomizable)
    set_randomization, set_reset_randomization, reset_randomization, set_noise_sigmas, apply_reset_randomization, clear_randomization
                                    dr.Randomizable's, on the handle that owns the tables
    set_gravity(z), base_gravity_z  base_gravity_z: the task's own gravity, what a randomised gravity scales or offsets; set_gravity
                                    does not change it
    control_dt                      seconds per control step, read when asked
    joint_limits()                  (float32 [num_dofs, 4]: lower, upper, effort, vel_limit; the joint names) of the model the step runs
    joint_views()                   (q, qd, tau) as [num_envs, num_dofs] float32 views of the env's own tensors, any strides
    step(actions), reset_all(), reset_idx(env_ids)
    set_serve_plan, apply_serve_plan, clear_serve_plan, serve_defaults, serve_plan   (include/ppenv_serve.h)
    set_serve_curriculum, clear_serve_curriculum, serve_curriculum, serve_target()   (include/ppenv_serve_curric.h; a plan and a curriculum
                                    write the same override buffer and cannot coexist)"""
    serve_curriculum = None

    def set_serve_curriculum(self, bins, power=1, mix=0.25, alpha=0.3, seed=None, horizon=32):
        """An adaptive serve curriculum (include/ppenv_serve_curric.h; curriculum.ServeCurriculum has the arguments): from now on every reset
        inside a step serves the ball the curriculum last drew for that env, and the caller launches curriculum.step(t, rew, reset) once after
        every step, fold() and update() once per horizon.  Switches the override exactly as set_serve_plan does — for the 7-dof handles BY
        VALUE in the step kernel's arguments: a graph captured before this call must be captured again.  With a serve plan set: ValueError.
        -> the ServeCurriculum."""
        if self.serve_plan is not None:
            raise ValueError("a serve plan is set: a plan and a curriculum write the same override buffer; call clear_serve_plan() first")
        from .curriculum import ServeCurriculum
        cur = ServeCurriculum(self, bins, power=power, mix=mix, alpha=alpha, seed=seed, horizon=horizon)
        self._serve_override_switch(True)
        self.serve_curriculum = cur
        return cur

    def clear_serve_curriculum(self):
        """The built-in serves again, as after clear_serve_plan."""
        if self.serve_curriculum is not None:
            self._serve_override_switch(False)
            self.serve_curriculum = None

    def _refuse_plan_beside_curriculum(self):
        if self.serve_curriculum is not None:
            raise ValueError("a serve curriculum is set: a plan and a curriculum write the same override buffer; call clear_serve_curriculum() first")

    def apply_serve_plan(self, env_ids=None):
        """The per-step launch (pp_serve_apply on reset_buf), once after every step while a plan is set; env_ids: the id variant, after
        reset_idx(env_ids) (all envs: an arange).  No synchronisation; capturable."""
        if self.serve_plan is None:
            raise _lib.PPEnvError("apply_serve_plan: no plan is set (set_serve_plan)")
        if env_ids is None:
            self.serve_plan.apply(self.reset_buf)
        else:
            self.serve_plan.apply_ids(env_ids)
