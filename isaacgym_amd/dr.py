"""Reset-time, per-env domain randomisation drawn on the device (include/ppenv_dr.h): the tables, the uploaded plan and the state
block of one environment handle, and the two launches.  The reference's rule — an env's actor parameters are redrawn when THAT env
resets (tasks/humanoid_pingpong_3_actor_tilt.py:849-850, 1025; upstream VecTask.apply_randomizations) — without a host round trip.
torch owns the memory, as it owns the environments' arenas; the library rewrites table columns in place."""
import ctypes as C

import torch

from . import _lib, scene


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
            _lib.check(L.ppenv_dr_plan_upload(C.byref(host), self.plan_dev.data_ptr(), self._stream()), L)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def apply(self, reset_buf):
        """One control step of the rule (ppenv_dr_apply), after the step that wrote reset_buf [reset_rows * N] int64.  One launch, no
        synchronisation."""
        assert reset_buf.dtype == torch.int64 and reset_buf.is_contiguous() and reset_buf.numel() == self.reset_rows * self.num_envs
        _lib.check(self.L.ppenv_dr_apply(self.plan_dev.data_ptr(), self.num_envs, reset_buf.data_ptr(), self.randomize_buf.data_ptr(),
                                         self.state.data_ptr(), self._stream()), self.L)

    def apply_ids(self, env_ids):
        """The rule for the envs reset_idx(env_ids) lists (ppenv_dr_apply_ids); duplicates are dropped here (the kernel wants distinct ids)."""
        ids = torch.unique(torch.as_tensor(env_ids, dtype=torch.int64).reshape(-1).to(self.device))
        if ids.numel() == 0:
            return
        _lib.check(self.L.ppenv_dr_apply_ids(self.plan_dev.data_ptr(), self.num_envs, ids.data_ptr(), ids.numel(), self.randomize_buf.data_ptr(),
                                             self.state.data_ptr(), self._stream()), self.L)
        ids.record_stream(torch.cuda.current_stream(self.device))
