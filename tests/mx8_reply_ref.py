"""numpy restatement of MX8 replies (include/fedavg/fa.h, "MX8 replies", rules 1-6) on top of tests/mx8_ref.py.

Not a test module.  A reply is ``encode(widen(y) - widen(sent))`` followed by ``expand`` against ``sent``: the deltas
are one fp32 subtract each, the blocks those of the whole bucket (``idx0`` shifts a range into it), the model the
owners then hold is decode rule 3.  bf16 values travel as ``np.uint16`` bit patterns, fp16 as ``np.float16``.
"""
import numpy as np

import mx8_ref as M

F32, U8 = np.float32, np.uint8


def deltas(y, sent, kind):
    """Rule 3: delta_i = fl32(widen(y_i) - widen(sent_i))."""
    with np.errstate(all="ignore"):
        return (M.widen(y, kind) - M.widen(sent, kind)).astype(F32)


def encode_range(delta, idx0=0):
    """Encode rules 1-3 over bucket elements [idx0, idx0 + n): (q, e), e[0] the scale of block idx0 >> 5 from the
    elements of the range alone (zeros before idx0 change neither a block's maximum nor its finiteness)."""
    lead = idx0 & 31
    q, e = M.encode(np.concatenate([np.zeros(lead, F32), np.ascontiguousarray(delta, F32)]))
    return q[lead:].copy(), e


def codes_under(delta, e, idx0=0):
    """Encode rule 3's codes under given scales (rule 6: a block's scale may come from beyond the range)."""
    t = np.asarray(e, np.int64)[M.block_of(delta.size, idx0)] - 133
    with np.errstate(all="ignore"):
        scaled = np.ldexp(np.where(t == 122, 0.0, np.ascontiguousarray(delta, F32).astype(np.float64)), (-t).astype(np.int32))
    return np.clip(np.rint(scaled), -127, 127).astype(np.int8)


def reply(y, sent, kind, idx0=0):
    """Rules 3-4 over one range: (q, e, g')."""
    q, e = encode_range(deltas(y, sent, kind), idx0)
    return q, e, M.expand(q, e, idx0, kind, sent, kind)


class Owners:
    """Rules 1-5 chained over rounds: what the library's part state must be after each reducing call."""

    def __init__(self, kind):
        self.kind, self.sent = kind, None

    def round(self, y):
        """y: the part's output without the stage.  Returns (q, e, output); q and e are None in the bootstrap."""
        if self.sent is None:
            self.sent = np.array(y, copy=True)
            return None, None, self.sent
        q, e, g = reply(y, self.sent, self.kind)
        self.sent = g
        return q, e, g
