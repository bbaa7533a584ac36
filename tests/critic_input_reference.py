"""The privileged critic inputs restated in numpy from the words of include/ppenv_critic_input.h — not from the kernels.  The GPU tests
compare the launches against these bit for bit.

A source is a dict(array=, table_major=): a ROW-MAJOR array [rows, cols] (or [rows]: one column; any view of a wider array: the row stride
is the view's), or a TABLE-MAJOR array [cols, num_envs] (or [num_envs]: one column).  float32 is copied bit for bit, int32 converted."""
import numpy as np


def widths(sources):
    return [1 if s["array"].ndim == 1 else (s["array"].shape[0] if s["table_major"] else s["array"].shape[1]) for s in sources]


def gather(sources, rows, num_agents):
    """out[r, off_s + c] = element (r, c) of a row-major source, element (c, r // A) of a table-major one; the sources' columns follow one
    another in table order.  -> float32 [rows, P]."""
    out = np.zeros((rows, sum(widths(sources))), np.float32)
    env = np.arange(rows) // num_agents                          # e(r) = r / A: env e owns rows A e .. A e + A - 1
    off = 0
    for s, w in zip(sources, widths(sources)):
        a = s["array"]
        assert a.dtype in (np.float32, np.int32)
        if s["table_major"]:
            a = a.reshape(w, -1)
            assert a.shape[1] * num_agents == rows
            block = a[:, env].T                                  # [rows, w]
        else:
            block = a.reshape(rows, w)
        if a.dtype == np.int32:
            block = block.astype(np.float32)                     # C's conversion: round to nearest even
            out[:, off:off + w] = block
        else:
            out[:, off:off + w].view(np.uint32)[...] = np.ascontiguousarray(block).view(np.uint32)      # bit for bit
        off += w
    return out


def prepare(x16, priv, mean, inv_std, clip, col0):
    """x16 [rows, ld] float16, IN PLACE: columns col0 .. col0 + P = fp16(clamp((priv - mean) * inv_std, -clip, clip)), every operation
    rounded to float32 on its own, the fp16 rounding to nearest even (mean None: converted only); columns col0 + P .. ld = 0; columns
    below col0 untouched."""
    rows, P = priv.shape
    assert x16.dtype == np.float16 and priv.dtype == np.float32 and col0 >= 0 and col0 + P <= x16.shape[1]
    v = priv
    if mean is not None:
        d = (priv - mean.astype(np.float32)).astype(np.float32)
        v = np.minimum(np.maximum((d * inv_std.astype(np.float32)).astype(np.float32), np.float32(-clip)), np.float32(clip))
    x16[:, col0:col0 + P] = v.astype(np.float16)
    x16[:, col0 + P:] = 0
    return x16
