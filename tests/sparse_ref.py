"""The sparse-sum stage (fa.h "Sparse-sum stage", rules 1-2) restated in plain numpy with an exact fmaf: the product of two
fp32 values is exact in fp64, the add is made with TwoSum and rounded to odd at 53 bits, one rounding to fp32 follows (53 >=
2 * 24 + 2, so the two roundings are one).  The tests compare libfa's host function and its kernels against this, every
bit."""
import numpy as np

from mx8_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)

F32, F64, U32 = np.float32, np.float64, np.uint32


def fmaf(w, d, acc):
    """fl32(w * d + acc), one rounding, elementwise over fp32 arrays (w may be a scalar)."""
    with np.errstate(all="ignore"):
        p = np.asarray(w, F32).astype(F64) * np.asarray(d, F32).astype(F64)  # exact: 24 x 24 bits
        a = np.asarray(acc, F32).astype(F64)
        s = p + a
        t = s - p  # TwoSum: s + e == p + a exactly
        e = (p - (s - t)) + (a - t)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)  # inexact and even: the odd neighbour
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def sparse_sum(idx, val, w, n, idx0=0, g=None):
    """a fp32[n] over bucket elements idx0 .. idx0 + n - 1: rule 1 client by client (which is every element's chain in
    ascending client order; a client's indices are distinct), then rule 2 against g, the widened reference, or None."""
    acc = np.zeros(n, F32)
    for c in range(len(idx)):
        e = np.asarray(idx[c], np.int64) - idx0
        m = (e >= 0) & (e < n)
        acc[e[m]] = fmaf(F32(w[c]), np.asarray(val[c], F32)[m], acc[e[m]])
    if g is None:
        return acc
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(g, F32) + acc).astype(F32)


def receipts(D, bucket, k_most, seed, empty=()):
    """D top-k receipts over a bucket: k_c random in k_most / 2 .. k_most (0 for the clients in `empty`), idx ascending."""
    rng = np.random.default_rng(seed)
    idx, val = [], []
    for c in range(D):
        k = 0 if c in empty else int(rng.integers(min(k_most, bucket) // 2, min(k_most, bucket) + 1))
        idx.append(np.sort(rng.choice(bucket, k, replace=False)).astype(U32))
        val.append(rng.standard_normal(k).astype(F32))
    return idx, val


def with_entries(idx, val, at, seed):
    """The receipts with an entry planted at every bucket position of `at` (kept ascending, the planted value wins)."""
    rng = np.random.default_rng(seed)
    at = np.unique(np.asarray(at, np.int64))
    out_i, out_v = [], []
    for i, v in zip(idx, val):
        keep = ~np.isin(i, at)
        ai = np.concatenate([i[keep].astype(np.int64), at])
        av = np.concatenate([v[keep], rng.standard_normal(at.size).astype(F32)])
        o = np.argsort(ai, kind="stable")
        out_i.append(ai[o].astype(U32))
        out_v.append(av[o].astype(F32))
    return out_i, out_v
