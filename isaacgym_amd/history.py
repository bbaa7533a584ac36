"""Observation and action history for the actor: a frame stack kept on the device (C ABI and the rule in full: include/ppenv_history.h;
DESIGN §5d "Observation and action history").

Training under control latency and randomisation hides state from the policy: its observation may be several control steps old, by a
delay drawn per episode, and an env's masses and gains change at every reset.  A memoryless MLP over one observation cannot infer either.
With a history (Ho, Ha) the policy's input row becomes

    wide = [ o_0 | o_1 | .. | o_Ho | a_1 | .. | a_Ha ]          W = (Ho + 1) * n + Ha * A

the observation it sees now, the Ho it saw before, and its own last Ha clamped commands.  One launch per control step builds the next
wide row from the previous one (`HistoryStack.push`); a row whose env has just reset holds its first observation in every slot and has
zero actions, so nothing is carried across a reset.  The rule is this build's own specification — no reference pins it; `reference`
restates it in numpy and the tests compare the kernel against that bit for bit.

`parse`, `bind`, `check_record`, `text` and `reference` are host-only."""
import numpy as np
import torch

from . import _lib

MAX, MAX_WIDTH = _lib.HISTORY_MAX, _lib.HISTORY_MAX_WIDTH
LO, HI = -1.0, 1.0                         # the clamp of a stored action: the sampler's and RLGamesPolicy.act's


def _whole(x):
    if isinstance(x, bool) or not isinstance(x, (int, float, str)) and not hasattr(x, "__index__"):
        raise ValueError
    if isinstance(x, str):
        return int(x.strip(), 10)
    if float(x) != int(x):
        raise ValueError
    return int(x)


def parse(spec, num_obs=None, num_actions=None):
    """The `history` argument -> None (no history) or a record.  spec: None; a (Ho, Ha) pair; dict(obs=Ho, actions=Ha) — a checkpoint's
    record is one, its other keys are checked against the task when one is bound —; or the CLI's text "Ho,Ha" / "Ho:Ha".  (0, 0) is None:
    the two CLI flags default to 0.  Ho and Ha are whole numbers in 0 .. MAX; anything else is a ValueError naming the argument.
    With num_obs = n and num_actions = A the record is bound to a task: dict(obs=Ho, actions=Ha, num_obs=n, num_actions=A, width=W), and a W
    above MAX_WIDTH is refused; without them: dict(obs=Ho, actions=Ha)."""
    if spec is None:
        return None
    try:
        if isinstance(spec, dict):
            if set(spec) - {"obs", "actions", "num_obs", "num_actions", "width"} or "obs" not in spec or "actions" not in spec:
                raise ValueError
            ho, ha = _whole(spec["obs"]), _whole(spec["actions"])
        elif isinstance(spec, str):
            parts = spec.replace(":", ",").split(",")
            if len(parts) != 2:
                raise ValueError
            ho, ha = _whole(parts[0]), _whole(parts[1])
        elif isinstance(spec, (tuple, list)):
            if len(spec) != 2:
                raise ValueError
            ho, ha = _whole(spec[0]), _whole(spec[1])
        else:
            raise ValueError
        if not (0 <= ho <= MAX and 0 <= ha <= MAX):
            raise ValueError
    except (ValueError, TypeError, OverflowError):
        raise ValueError(f"history: a history is (Ho, Ha), dict(obs=Ho, actions=Ha) or the text 'Ho,Ha': whole numbers of earlier observations and "
                         f"earlier actions, each 0 .. {MAX}, not {spec!r}") from None
    if ho == 0 and ha == 0:
        return None
    rec = dict(obs=ho, actions=ha)
    if num_obs is None and num_actions is None:
        return rec
    return bind(rec, num_obs, num_actions, spec if isinstance(spec, dict) else None)


def width(num_obs, num_actions, obs, actions):
    """W = (Ho + 1) * n + Ha * A — pp_history_width's arithmetic without the library (0: refused)."""
    n, a, ho, ha = int(num_obs), int(num_actions), int(obs), int(actions)
    if n < 1 or a < 1 or not 0 <= ho <= MAX or not 0 <= ha <= MAX or ho == ha == 0:
        return 0
    w = (ho + 1) * n + ha * a
    return 0 if w > MAX_WIDTH else w


def bind(rec, num_obs, num_actions, stored=None):
    """dict(obs=, actions=) and a task's n and A -> the full record.  stored: a record that already names num_obs / num_actions / width (a
    checkpoint's): it must agree."""
    n, a = int(num_obs), int(num_actions)
    w = width(n, a, rec["obs"], rec["actions"])
    if w == 0:
        raise ValueError(f"history: {rec['obs']} observations + {rec['actions']} actions back of {n} observations and {a} actions make a first layer wider "
                         f"than {MAX_WIDTH} columns (or n, A below 1)")
    out = dict(obs=int(rec["obs"]), actions=int(rec["actions"]), num_obs=n, num_actions=a, width=w)
    if stored is not None:
        for k in ("num_obs", "num_actions", "width"):
            if k in stored and int(stored[k]) != out[k]:
                raise ValueError(f"history: the record {dict(stored)} was made for {k} = {int(stored[k])}, here {k} = {out[k]}")
    return out


def check_record(theirs, mine):
    """load(): a checkpoint's record against the trainer's (either may be None: no history).  ValueError naming both."""
    key = lambda r: None if r is None else (int(r["obs"]), int(r["actions"]), int(r.get("num_obs", -1)), int(r.get("num_actions", -1)))
    if key(theirs) != key(mine):
        say = lambda r: "no history" if r is None else f"history {dict(r)}"
        raise ValueError(f"history: the checkpoint was trained with {say(theirs)}, this trainer has {say(mine)}")


def text(rec):
    """The trainer's start-up line."""
    pad = lambda k: (k + 63) // 64 * 64
    return (f"history: {rec['obs']} observations + {rec['actions']} actions back: first layer K {rec['num_obs']} -> {rec['width']} "
            f"(padded {pad(rec['width'])})")


def reference(prev, obs, act, done, num_obs, num_actions, obs_back, actions_back, num_agents=1, lo=LO, hi=HI):
    """The rule of include/ppenv_history.h in numpy.  prev: float32 [rows, >= W] or None; obs [rows, >= n]; act [rows, >= A] or None where it
    is not read; done: int64 [rows] or None.  -> float32 [rows, W].  Words are moved as uint32 views, so NaN payloads and the sign of a zero
    survive; the clamp is fmin(fmax(x, lo), hi), which turns a NaN action into lo."""
    n, a, ho, ha = int(num_obs), int(num_actions), int(obs_back), int(actions_back)
    w = width(n, a, ho, ha)
    assert w > 0
    bits = lambda x: np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    o = bits(obs)[:, :n]
    rows = o.shape[0]
    assert rows % num_agents == 0
    start = np.ones(rows, bool)
    if prev is not None:
        start[:] = False
        if done is not None:
            d = np.asarray(done).astype(np.int64).reshape(rows // num_agents, num_agents)
            start = np.repeat(d[:, 0] != 0, num_agents)          # agent 0's word, all 64 bits, for every row of the env
    out = np.zeros((rows, w), np.uint32)
    out[:, :(ho + 1) * n] = np.tile(o, (1, ho + 1))              # a start: the first sample in every observation slot, zero actions
    keep = ~start
    if prev is not None and keep.any():
        p = bits(prev)[:, :w]
        e = (ho + 1) * n
        out[keep, n:e] = p[keep, :ho * n]
        if ha:
            x = np.asarray(act, np.float32)[:, :a]
            a1 = np.fmin(np.fmax(x, np.float32(lo)), np.float32(hi)).astype(np.float32)
            out[keep, e:e + a] = np.ascontiguousarray(a1).view(np.uint32)[keep]
            out[keep, e + a:] = p[keep, e:e + (ha - 1) * a]
    return out.view(np.float32)


class HistoryStack:
    """pp_history_push (include/ppenv_history.h) on torch tensors.  `push(obs, act, done, prev, out)` builds the wide rows `out`
    [rows, W] from `prev` [rows, W] (None: every row starts), the new observation `obs` [rows, n], the action `act` [rows, A] the policy
    issued on `prev` and that step's `done` ([rows] int64 or None); one launch, nothing synchronises, no state is kept here — the state
    is `prev` itself.  All matrices are float32 on this device with unit stride along the row and a row stride >= their width (a slice of
    a horizon buffer, the first columns of a wider tensor).

    For a player: `advance(obs, act, done)` pushes from the stack's current buffer into its other one and returns that — the wide tensor
    the policy reads now; `reset()` makes the next advance a prev = None push.  The two buffers are allocated at the first advance."""

    def __init__(self, rows, num_obs, num_actions, obs_back, actions_back, device, num_agents=1, lo=LO, hi=HI):
        self.rows, self.n, self.a, self.num_agents = int(rows), int(num_obs), int(num_actions), int(num_agents)
        self.obs_back, self.actions_back, self.lo, self.hi = int(obs_back), int(actions_back), float(lo), float(hi)
        self.width = width(self.n, self.a, self.obs_back, self.actions_back)
        if self.width == 0 or self.rows < 1 or self.num_agents not in (1, 2) or self.rows % self.num_agents or not self.lo <= self.hi:
            raise ValueError(f"HistoryStack: rows {rows} (>= 1, a multiple of num_agents), num_agents {num_agents} (1 or 2), {num_obs} observations, "
                             f"{num_actions} actions, history ({obs_back}, {actions_back}) (each 0 .. {MAX}, not both 0, at most {MAX_WIDTH} columns), "
                             f"lo {lo} <= hi {hi}")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:                       # tensors carry an index: compare like with like
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.L = _lib.lib()
        assert self.L.pp_history_width(self.n, self.a, self.obs_back, self.actions_back) == self.width
        self._buf, self._cur = None, -1                                    # advance()'s two buffers; -1: the next advance starts every row

    def record(self):
        return dict(obs=self.obs_back, actions=self.actions_back, num_obs=self.n, num_actions=self.a, width=self.width)

    def _matrix(self, name, t, cols):
        R = self.rows
        if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != (R, cols) or (cols > 1 and t.stride(1) != 1) or (R > 1 and t.stride(0) < cols):
            raise ValueError(f"HistoryStack.push: {name} must be float32 [{R}, {cols}] on {self.device} with unit stride along the row and a row stride >= {cols}")
        return t.data_ptr(), t.stride(0) if R > 1 else cols

    def push(self, obs, act, done, prev, out):
        """-> out.  act may be None where it is not read: prev is None, or no actions are kept."""
        (po, ldo), (pn, ldn) = self._matrix("obs", obs, self.n), self._matrix("out", out, self.width)
        pa, lda = (None, self.a) if act is None else self._matrix("act", act, self.a)
        pp, ldp = (None, self.width) if prev is None else self._matrix("prev", prev, self.width)
        if done is not None and (done.dtype != torch.int64 or done.numel() != self.rows or not done.is_contiguous() or done.device != self.device):
            raise ValueError(f"HistoryStack.push: done must be int64, contiguous [{self.rows}] on {self.device}, or None")
        _lib.check(self.L.pp_history_push(po, ldo, pa, lda, _lib.ptr(done), pp, ldp, pn, ldn, self.rows, self.num_agents, self.n, self.a, self.obs_back,
                                          self.actions_back, self.lo, self.hi, _lib.stream(self.device)), self.L)
        return out

    def reset(self):
        """The next advance() is a prev = None push: every row starts."""
        self._cur = -1

    def advance(self, obs, act, done):
        """One control step of a player: -> the wide tensor [rows, W] the policy reads now (valid until the advance after the next)."""
        if self._buf is None:
            self._buf = torch.zeros((2, self.rows, self.width), dtype=torch.float32, device=self.device)
        if self._cur < 0:
            self._cur = 0
            return self.push(obs, None, None, None, self._buf[0])
        nxt = 1 - self._cur
        self.push(obs, act, done, self._buf[self._cur], self._buf[nxt])
        self._cur = nxt
        return self._buf[nxt]
