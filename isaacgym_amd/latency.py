"""Control latency during training: the delay line whose per-row delay is redrawn on the device at every episode start (DelayLine; C ABI
and the rule in full: include/ppenv_train_delay.h), and the parsing of a latency argument (an int K, a (lo, hi) pair, the CLI's "K" or
"LO:HI").  The rule is this build's own specification — the reference delays nothing and no oracle pins it.  play.accounting.Delay is the
player's line, with a per-row table the host uploads; RolloutCollector / PPOTrainer(action_delay=, obs_delay=) use this one."""
import ctypes as C

import torch

from . import _lib

DELAY_MAX, DELAY_MAX_WIDTH = _lib.PLAY_DELAY_MAX, _lib.PLAY_DELAY_MAX_WIDTH
COMMAND, SENSING = 0, 1                    # PP_TRAIN_DELAY_COMMAND, PP_TRAIN_DELAY_SENSING


def delay_range(name, value):
    """A latency argument -> (lo, hi), whole control steps with 0 <= lo <= hi <= DELAY_MAX: an int K is (K, K); a (lo, hi) pair of ints; the
    text "K" or "LO:HI" (the CLI's).  Anything else — negative, lo > hi, above DELAY_MAX, a fraction, a bool — raises ValueError naming
    `name`."""
    def whole(x):
        if isinstance(x, bool) or not isinstance(x, (int, float, str)) and not hasattr(x, "__index__"):
            raise ValueError
        if isinstance(x, str):
            return int(x.strip(), 10)
        if float(x) != int(x):
            raise ValueError
        return int(x)
    try:
        if isinstance(value, str):
            parts = value.split(":")
            if len(parts) not in (1, 2):
                raise ValueError
            lo, hi = (whole(parts[0]),) * 2 if len(parts) == 1 else (whole(parts[0]), whole(parts[1]))
        elif isinstance(value, (tuple, list)):
            if len(value) != 2:
                raise ValueError
            lo, hi = whole(value[0]), whole(value[1])
        else:
            lo = hi = whole(value)
        if not 0 <= lo <= hi <= DELAY_MAX:
            raise ValueError
    except (ValueError, TypeError, OverflowError):
        raise ValueError(f"{name}: a delay is a number of whole control steps K or a range LO:HI / (lo, hi) with 0 <= lo <= hi <= {DELAY_MAX}, "
                         f"not {value!r}") from None
    return lo, hi


def latency_text(lat):
    """dict(control_dt, action_delay=[lo, hi], obs_delay=[lo, hi]) -> the trainer's start-up line: steps and milliseconds, as play's
    `latency:` line."""
    ms = 1000.0 * lat["control_dt"]

    def one(r):
        lo, hi = r
        return f"{lo} steps = {lo * ms:.6g} ms" if lo == hi else f"{lo}..{hi} steps = {lo * ms:.6g}..{hi * ms:.6g} ms, drawn per episode"
    return f"latency: control dt {ms:.6g} ms; " + "; ".join(f"{axis} {one(lat[axis])}" for axis in ("action_delay", "obs_delay"))


class DelayLine:
    """pp_train_delay_reset / pp_train_delay_push (include/ppenv_train_delay.h) on torch tensors: a delay line of whole control steps for
    a [rows, width] float32 tensor whose per-row delay is drawn on the device in lo .. hi at every episode start, keyed (seed, env_id_offset +
    env, the row's episode count, channel) — scene.latency_draws predicts it.  push(x, done, out) stores this control step's sample and
    writes to `out` the one delays[r] steps old of the same episode, or the episode's first sample while there is none that old; `done`
    ([rows] int64, the done the previous env step returned, or None right after reset()) marks the sample as the first of a new episode of
    its env (agent 0's word).  It owns the ring [hi + 1, rows, width], `age`, `episode` and `delays` (device int32 [rows], written by the
    kernel); x is not modified.  `seed` is a STREAM seed.  One launch per push, nothing here synchronises."""

    def __init__(self, rows, width, lo, hi, device, num_agents=1, seed=0, env_id_offset=0, channel=COMMAND):
        self.rows, self.width, self.num_agents = R, W, A = int(rows), int(width), int(num_agents)
        if R < 1 or A not in (1, 2) or R % A or not 1 <= W <= DELAY_MAX_WIDTH:
            raise ValueError(f"DelayLine: rows {rows} (>= 1, a multiple of num_agents), num_agents {num_agents} (1 or 2), width {width} (1..{DELAY_MAX_WIDTH})")
        self.lo, self.hi = delay_range("DelayLine: (lo, hi)", (lo, hi))
        if channel not in (COMMAND, SENSING):
            raise ValueError(f"DelayLine: channel {channel!r} is not 0 (the command path) or 1 (the sensing path)")
        self.seed, self.env_id_offset, self.channel = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_offset), int(channel)
        if not 0 <= self.env_id_offset <= 2 ** 31 - 1 - R // A:
            raise ValueError(f"DelayLine: env_id_offset {env_id_offset} (>= 0; the last env's id below 2^31)")
        self.depth = self.hi + 1
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:                       # tensors carry an index: compare like with like
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        L = self.L = _lib.lib()
        self._consts = _lib.TrainDelayConsts(self.lo, self.hi, self.seed, self.env_id_offset, self.channel)
        self.delays = torch.zeros(R, dtype=torch.int32, device=dev)
        self.age = torch.zeros(R, dtype=torch.int32, device=dev)
        self.episode = torch.zeros(R, dtype=torch.int32, device=dev)
        self.ring = torch.zeros((self.depth, R, W), dtype=torch.float32, device=dev)
        assert self.ring.numel() * 4 == L.pp_train_delay_ring_bytes(R, W, self.hi) and 4 * R == L.pp_train_delay_table_bytes(R)
        self.reset()

    def reset(self):
        """age and episode to zero: every row's next sample is the first of its episode 0."""
        _lib.check(self.L.pp_train_delay_reset(self.rows, self.age.data_ptr(), self.episode.data_ptr(), _lib.stream(self.device)), self.L)

    def _matrix(self, name, t):
        R, W = self.rows, self.width
        if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != (R, W) or (W > 1 and t.stride(1) != 1) or (R > 1 and t.stride(0) < W):
            raise ValueError(f"DelayLine.push: {name} must be float32 [{R}, {W}] on {self.device} with unit stride along the row and a row stride >= {W}")
        return t.data_ptr(), t.stride(0) if R > 1 else W

    def push(self, x, done, out):
        """x, out: float32 [rows, width] on this device, unit stride along the row and a row stride >= width (contiguous tensors, or the
        first `width` columns of wider ones), not overlapping; done: [rows] int64 contiguous, or None.  -> out."""
        (px, ldx), (po, ldo) = self._matrix("x", x), self._matrix("out", out)
        if done is not None and (done.dtype != torch.int64 or done.numel() != self.rows or not done.is_contiguous() or done.device != self.device):
            raise ValueError(f"DelayLine.push: done must be int64, contiguous [{self.rows}] on {self.device}, or None")
        _lib.check(self.L.pp_train_delay_push(px, ldx, _lib.ptr(done), self.rows, self.num_agents, self.width, C.byref(self._consts), self.delays.data_ptr(),
                                              self.age.data_ptr(), self.episode.data_ptr(), self.ring.data_ptr(), po, ldo, _lib.stream(self.device)), self.L)
        return out
