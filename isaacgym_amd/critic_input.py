"""Privileged critic inputs: what an env hides from the policy, shown to the critic alone (C ABI and the layout in full:
include/ppenv_critic_input.h; DESIGN §5d "Privileged critic inputs").

Training under domain randomisation and control latency hides state from the network: an env's masses, gains, friction and restitution
change at every reset, its delays at every episode start, and with an observation delay the observation is several control steps old.
The actor has to cope with that.  The critic exists only during training, and a value function that cannot see which physics an env has
averages over them — variance that goes straight into the advantages.  OpenAI's ADR work and DeXtreme train an asymmetric actor-critic
for this reason.  Here every privileged quantity is on the device already; `CriticInput` gathers the named ones into one fp32 row per
actor row, one launch per control step, straight into the collector's horizon slice (RolloutCollector(critic_input=),
PPOTrainer(critic_inputs=), --critic-inputs).

The source NAMES, in the order the caller gives them; each contributes consecutive columns:

    tables    every table of env.dr_tables that is set, in dr.TABLE_NAMES order, one column per table row (a per-env scalar: one column).
              Table-major sources: actor row r reads env r // num_agents, so both rows of a 4-actor env see the same columns.
    latency   act_line.delays and / or obs_line.delays (int32, converted), command path first, for the lines that exist
    raw_obs   the collector's undelayed observation `raw_obs` (it exists with an obs_delay line)

`resolve` and the record functions are host-only and run on CPU tensors; `CriticInput` owns the uploaded table and the launch.
"""
import ctypes as C
import dataclasses

import torch

from . import _lib, dr

NAMES = ("tables", "latency", "raw_obs")
MAX_SOURCES, MAX_COLS = _lib.CRITIC_MAX_SOURCES, _lib.CRITIC_MAX_COLS


@dataclasses.dataclass
class Source:
    """One entry of the source table (pp_critic_source): `tensor` float32 or int32; row-major [rows, cols] (or [rows]: one column) with
    `stride` elements between rows, or table-major [cols, num_envs] (or [num_envs]) with `stride` elements between table rows."""
    name: str                  # the NAME it was resolved for
    label: str                 # which tensor: a table's name, "action_delay", "obs_delay", "raw_obs"
    tensor: torch.Tensor
    cols: int
    table_major: bool
    stride: int

    @property
    def kind(self):
        return _lib.CRITIC_I32 if self.tensor.dtype == torch.int32 else _lib.CRITIC_F32


def source(name, label, tensor, table_major):
    """A Source of a tensor as it lies in memory.  Refuses (ValueError) another dtype than float32 / int32, more than two dimensions, and
    an inner stride other than 1."""
    t = tensor
    if t.dtype not in (torch.float32, torch.int32) or t.dim() not in (1, 2) or t.stride(-1) != 1 and t.shape[-1] > 1:
        raise ValueError(f"critic_inputs: {label} must be a float32 or int32 tensor of one or two dimensions with unit inner stride")
    if table_major:
        cols, stride = (1, t.shape[0]) if t.dim() == 1 else (t.shape[0], t.stride(0) if t.shape[0] > 1 else t.shape[1])
    else:
        cols, stride = (1, 1) if t.dim() == 1 else (t.shape[1], t.stride(0) if t.shape[0] > 1 else t.shape[1])
    return Source(name, label, t, int(cols), bool(table_major), int(stride))


def parse(names):
    """The `critic_inputs` argument — a tuple / list of NAMES, or the CLI's comma-separated text — -> a tuple of names, in the given order.
    An unknown or a repeated name is a ValueError naming the argument."""
    if names is None:
        return ()
    if isinstance(names, str):
        names = [n.strip() for n in names.split(",") if n.strip()]
    names = tuple(names)
    for n in names:
        if n not in NAMES:
            raise ValueError(f"critic_inputs: {n!r} is not one of {', '.join(NAMES)}")
    if len(set(names)) != len(names):
        raise ValueError(f"critic_inputs: a name is given twice in {list(names)}")
    return names


def resolve(env, collector_lines, names):
    """Source names -> the list of Sources, in column order.  env: what has `dr_tables`; collector_lines: what has `act_line`, `obs_line`
    (latency.DelayLine or None) and `raw_obs` — a RolloutCollector.  Each refusal is a ValueError naming the argument:
    `tables` when the run has no randomisation, `latency` when neither line exists, `raw_obs` without an obs_delay line."""
    out = []
    for name in parse(names):
        if name == "tables":
            tabs = env.dr_tables
            if tabs is None or all(t is None for t in tabs):
                raise ValueError("critic_inputs: 'tables' needs a run with randomisation (randomization= or adr=; --randomize or --adr): "
                                 "this env has no randomisation tables")
            out += [source(name, label, t, True) for label, t in zip(dr.TABLE_NAMES, tabs) if t is not None]
        elif name == "latency":
            lines = [(label, line) for label, line in (("action_delay", collector_lines.act_line), ("obs_delay", collector_lines.obs_line)) if line is not None]
            if not lines:
                raise ValueError("critic_inputs: 'latency' needs a delay line (action_delay= or obs_delay= above 0; --action-delay or --obs-delay): "
                                 "this run has neither")
            out += [source(name, label, line.delays, False) for label, line in lines]
        else:
            if collector_lines.obs_line is None or collector_lines.raw_obs is None:
                raise ValueError("critic_inputs: 'raw_obs' needs an obs_delay line (obs_delay= above 0; --obs-delay): without one the policy "
                                 "already sees the undelayed observation")
            out.append(source(name, "raw_obs", collector_lines.raw_obs, False))
    total = sum(s.cols for s in out)
    if len(out) > MAX_SOURCES or total > MAX_COLS:
        raise ValueError(f"critic_inputs: {len(out)} sources of {total} columns in all (at most {MAX_SOURCES} sources and {MAX_COLS} columns)")
    return out


def columns(names, table_rows, tables_set, action_delay, obs_delay, num_obs):
    """The record of `names` from what is known BEFORE the collector exists (PPOTrainer sizes the network with it): table_rows the env's
    DR_TABLE_ROWS, tables_set the names of the tables that are set (None: no randomisation), the two delay ranges (lo, hi), num_obs.
    The same refusals as resolve, through the same function."""
    class _Line:
        delays = torch.zeros(1, dtype=torch.int32)
    tabs = None if tables_set is None else [torch.zeros((max(table_rows[k], 1), 1)) if k in tables_set else None for k in dr.TABLE_NAMES]
    env = type("_Env", (), {"dr_tables": tabs})
    lines = type("_Lines", (), {"act_line": _Line if action_delay[1] > 0 else None, "obs_line": _Line if obs_delay[1] > 0 else None,
                                "raw_obs": torch.zeros((1, num_obs)) if obs_delay[1] > 0 else None})
    return record(resolve(env, lines, names))


def record(sources):
    """What a checkpoint keeps under "critic_inputs": the names in order, each name's column count, and P."""
    names = []
    for s in sources:
        if s.name not in names:
            names.append(s.name)
    return {"names": names, "columns": [sum(s.cols for s in sources if s.name == n) for n in names], "P": sum(s.cols for s in sources)}


def check_record(theirs, mine):
    """load(): a checkpoint's record against the trainer's (either may be None: no critic inputs).  ValueError saying which differs."""
    none = {"names": [], "columns": [], "P": 0}
    a, b = theirs or none, mine or none
    if int(a["P"]) != int(b["P"]):
        raise ValueError(f"critic_inputs: the checkpoint was trained with P = {int(a['P'])} privileged columns ({list(a['names'])}), this trainer has "
                         f"P = {int(b['P'])} ({list(b['names'])})")
    if list(a["names"]) != list(b["names"]) or [int(c) for c in a["columns"]] != [int(c) for c in b["columns"]]:
        raise ValueError(f"critic_inputs: the checkpoint's names {list(a['names'])} with columns {list(a['columns'])} are not this trainer's "
                         f"{list(b['names'])} with columns {list(b['columns'])}")


def text(rec, num_obs):
    """The trainer's start-up line."""
    pad = lambda k: (k + 63) // 64 * 64
    parts = " + ".join(f"{n} {c}" for n, c in zip(rec["names"], rec["columns"]))
    return f"critic inputs: {parts} = {rec['P']} columns (first layer K {pad(num_obs)} -> {pad(num_obs + rec['P'])})"


class CriticInput:
    """The uploaded source table of one env and collector, and the gather launch.  `gather(out)` writes the fp32 privileged rows
    out [rows, P] (unit inner stride, any row stride: a slice of a horizon buffer) as the sources stand at this point of the stream; one
    launch, nothing synchronises.  The table holds the sources' ADDRESSES: the tensors are kept alive here, and a source that is
    replaced rather than rewritten in place (env.set_randomization with new tensors, trainer.clear_randomization()) keeps being read
    where it was."""

    def __init__(self, env, collector_lines, names):
        self._build(resolve(env, collector_lines, names), env.num_rows, env.num_agents, env.device)

    @classmethod
    def from_sources(cls, sources, rows, num_agents, device):
        self = object.__new__(cls)
        self._build(list(sources), rows, num_agents, device)
        return self

    def _build(self, sources, rows, num_agents, device):
        self.sources, self.rows, self.num_agents = sources, int(rows), int(num_agents)
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.names = record(sources)["names"]
        self.P = sum(s.cols for s in sources)
        if not 1 <= len(sources) <= MAX_SOURCES:
            raise ValueError(f"critic_inputs: {len(sources)} sources (1 .. {MAX_SOURCES})")
        L = self.L = _lib.lib()
        host = _lib.CriticTable(rows=self.rows, num_agents=self.num_agents, sources=len(sources), total_cols=0)
        for i, s in enumerate(sources):
            if s.tensor.device != dev:
                raise ValueError(f"critic_inputs: {s.label} is on {s.tensor.device}, not on {dev}")
            host.source[i] = _lib.CriticSource(s.tensor.data_ptr(), s.kind, s.cols, _lib.CRITIC_TABLE_MAJOR if s.table_major else _lib.CRITIC_ROW_MAJOR, 0, s.stride)
        self.table_dev = torch.zeros(C.sizeof(_lib.CriticTable), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.pp_critic_input_upload(C.byref(host), self.table_dev.data_ptr(), _lib.stream(dev)), L)

    def record(self):
        return record(self.sources)

    def gather(self, out):
        if out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != (self.rows, self.P) or (self.P > 1 and out.stride(1) != 1) or \
                (self.rows > 1 and out.stride(0) < self.P):
            raise ValueError(f"CriticInput.gather: out must be float32 [{self.rows}, {self.P}] on {self.device} with unit stride along the row")
        _lib.check(self.L.pp_critic_input_gather(self.table_dev.data_ptr(), self.rows, self.num_agents, out.data_ptr(),
                                                 out.stride(0) if self.rows > 1 else self.P, _lib.stream(self.device)), self.L)
        return out
