"""numpy restatement of top-k receipts (include/fedavg/fa.h, "Top-k receipts"): decode, expansion and selection.

Not a test module.  It follows the rules, not the library: selection is a stable argsort of (-key, index), the sum and
the difference are numpy's fp32 operations.  bf16 values travel as ``np.uint16`` bit patterns, fp16 as ``np.float16``.
"""
import numpy as np

from mx8_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)

F32, U32 = np.float32, np.uint32
KINDS = {"f32": F32, "bf16": np.uint16, "f16": np.float16}
# key patterns that break a selector: each is the fp32 bit patterns of n deltas
PATTERNS = ["random", "equal", "two", "low digit", "high digit", "pm0", "zeros", "subnormal", "specials"]


def deltas(pattern, n, seed=0):
    rng = np.random.default_rng(seed)
    sign = rng.integers(0, 2, n).astype(U32) << U32(31)
    if pattern == "random":
        return rng.standard_normal(n).astype(F32)
    if pattern == "equal":  # the ties are cut purely by index
        return (np.full(n, 0x3FC00000, U32) | sign).view(F32)
    if pattern == "two":  # the cut falls inside either value's run, depending on k
        return np.where(rng.random(n) < 0.5, F32(2.0), F32(-0.5)).astype(F32)
    if pattern == "low digit":  # keys that differ only in the lowest 10 bits
        return (U32(0x3F800000) | rng.integers(0, 8, n).astype(U32) | sign).view(F32)
    if pattern == "high digit":  # ... and only in the highest 11
        return ((rng.integers(0x3F0, 0x3F8, n).astype(U32) << U32(20)) | sign).view(F32)
    if pattern == "pm0":  # +-0 only: every key equal, and zeros are selected like any value
        return (np.zeros(n, U32) | sign).view(F32)
    if pattern == "zeros":  # +-0 with a few non-zeros
        d = (np.zeros(n, U32) | sign).view(F32).copy()
        d[::7] = rng.standard_normal(d[::7].size).astype(F32)
        return d
    if pattern == "subnormal":
        return (rng.integers(0, 0x00800000, n).astype(U32) | sign).view(F32)
    d = rng.standard_normal(n).astype(F32)  # specials: NaN above inf above everything
    for i, v in enumerate([np.nan, np.inf, -np.inf, -np.nan, 1e-45, 0.0, -0.0]):
        d[(3 * i + 1) % n::23] = v
    return d


def select(delta, k):
    """Rules 2-5: (idx uint32[k'], val float32[k']) ascending in idx."""
    delta = np.ascontiguousarray(delta, F32).reshape(-1)
    key = (delta.view(U32) & U32(0x7FFFFFFF)).astype(np.int64)
    order = np.lexsort((np.arange(delta.size), -key))  # by -key, then by index
    idx = np.sort(order[:min(k, delta.size)])
    return idx.astype(U32), delta[idx]


def decode(idx, val, n, idx0=0):
    d = np.zeros(n, F32)
    at = np.asarray(idx, np.int64) - idx0
    ok = (at >= 0) & (at < n)
    d[at[ok]] = np.asarray(val, F32)[ok]
    return d


def expand(idx, val, n, idx0, slot_kind, g=None, ref_kind="f32"):
    """The slot (of slot_kind) from the entries and the reference g (of ref_kind; None: absolute)."""
    d = decode(idx, val, n, idx0)
    if g is None:
        return round_out(d, slot_kind)
    with np.errstate(all="ignore"):
        return round_out((widen(g, ref_kind) + d).astype(F32), slot_kind)


def encode(new, sent, kind, k):
    """Rules 1-6 on `new` and `sent` of one kind: (idx, val, g')."""
    with np.errstate(all="ignore"):
        delta = (widen(new, kind) - widen(sent, kind)).astype(F32)
    idx, val = select(delta, k)
    return idx, val, expand(idx, val, delta.size, 0, kind, sent, kind)
