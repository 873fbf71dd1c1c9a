"""numpy restatement of MX8 receipts (include/fedavg/fa.h, "MX8 receipts"): encode, decode and expand.

Not a test module.  It follows the rules, not the library: the scale is ``ldexp(1, E - 133)`` (the library builds
the bit pattern), the product and the sum are numpy's fp32 operations (IEEE, subnormals kept), the encoder scales in
fp64.  bf16 values travel as ``np.uint16`` bit patterns, fp16 as ``np.float16``.
"""
import numpy as np

from trimmed_ref import assert_bits, bf16_to_f32, f32_to_bf16  # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64
BLOCK = 32
E_EDGES = [0, 1, 6, 7, 126, 127, 133, 134, 253, 254, 255]
IDX0S = [0, 1, 31, 32, 33, 4097]


def scale_bytes(n):
    return (n + BLOCK - 1) // BLOCK


def scale(E):
    """Decode rule 2's s = 2^(E - 133) as fp32 (subnormal below E = 7); NaN for E = 255 (rule 1)."""
    E = np.asarray(E, np.int64)
    s = np.ldexp(F32(1.0), np.where(E == 255, 0, E - 133).astype(np.int32)).astype(F32)
    return np.where(E == 255, F32(np.nan), s).astype(F32)


def block_of(n, idx0=0):
    """Per element of [idx0, idx0 + n): the index into e, whose first byte scales block idx0 >> 5."""
    return ((np.arange(n, dtype=np.uint64) + np.uint64(idx0)) >> np.uint64(5)).astype(np.int64) - (idx0 >> 5)


def decode(q, e, idx0=0):
    """Decode rules 1-2: d_i = fl32((float)q_i * s), one multiply."""
    q = np.ascontiguousarray(q, np.int8)
    s = scale(np.ascontiguousarray(e, np.uint8)[block_of(q.size, idx0)])
    with np.errstate(all="ignore"):
        return (q.astype(F32) * s).astype(F32)


def widen(x, kind):
    if kind == "bf16":
        return bf16_to_f32(x)
    return np.ascontiguousarray(x).astype(F32)


def round_out(a, kind):
    a = np.ascontiguousarray(a, F32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16)
    if kind == "bf16":
        return f32_to_bf16(a)
    return a.copy()


def expand(q, e, idx0, slot_kind, g=None, ref_kind="f32"):
    """Decode rule 3: the slot (of slot_kind) from the codes and the reference g (of ref_kind; None: absolute)."""
    d = decode(q, e, idx0)
    if g is None:
        return round_out(d, slot_kind)
    with np.errstate(all="ignore"):
        return round_out((widen(g, ref_kind) + d).astype(F32), slot_kind)


def encode(delta):
    """Encode rules 1-3 over fp32 deltas: (q int8[n], e uint8[ceil(n / 32)])."""
    delta = np.ascontiguousarray(delta, F32).reshape(-1)
    n, B = delta.size, scale_bytes(delta.size)
    pad = np.zeros(B * BLOCK, F32)  # zeros change neither a block's maximum nor its finiteness
    pad[:n] = delta
    blk = pad.reshape(B, BLOCK)
    bad = ~np.isfinite(blk).all(axis=1)
    with np.errstate(all="ignore"):
        m = np.where(bad, F32(1.0), np.abs(blk).max(axis=1)).astype(F32)
    zero = m == 0
    f, k = np.frexp(np.where(zero, F32(1.0), m))  # m = f 2^k, f in [0.5, 1)
    t = np.where(f <= F32(127.0 / 128.0), k.astype(np.int64) - 7, k.astype(np.int64) - 6)
    E = np.clip(t + 133, 0, 254)
    t = E - 133
    with np.errstate(all="ignore"):
        scaled = np.ldexp(np.where(bad[:, None], 0.0, blk.astype(F64)), (-t).astype(np.int32)[:, None])
    q = np.clip(np.rint(scaled), -127, 127).astype(np.int8)
    q[bad | zero] = 0
    E = np.where(bad, 255, np.where(zero, 0, E)).astype(np.uint8)
    return q.reshape(-1)[:n].copy(), E


def error_bound(delta):
    """Encode rule 4, per element: max(m / 127, 2^-134) of its block, NaN for an E = 255 block (as fp64)."""
    delta = np.ascontiguousarray(delta, F32).reshape(-1)
    n, B = delta.size, scale_bytes(delta.size)
    pad = np.zeros(B * BLOCK, F32)
    pad[:n] = delta
    blk = pad.reshape(B, BLOCK).astype(F64)
    bad = ~np.isfinite(blk).all(axis=1)
    with np.errstate(all="ignore"):
        bound = np.maximum(np.abs(blk).max(axis=1) / 127.0, 2.0 ** -134)
    bound = np.where(bad, np.nan, bound)
    return np.repeat(bound, BLOCK)[:n]
