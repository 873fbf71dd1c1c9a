"""numpy restatement of the clip stage (include/fedavg/fa.h, "Clip stage"): the expected values of the clip tests.

Not a test module.  Rule 1 is computed exactly (``math.fsum`` of the fp64 squares: the stage's own summation
order is free, so the tests bound its error instead of fixing it); rules 2 and 3 are plain fp64 / fp32
arithmetic; rule 4 is the oracle's ordered FMA chain ``O.fedavg(xs, w', init=...)`` with the reference's term
``fl32(fma(c0, g, +0))`` as its start.  bf16 values travel as ``np.uint16`` bit patterns.
"""
import math

import numpy as np

from trimmed_ref import assert_bits, bf16_to_f32, f32_to_bf16  # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64


def widen(x, kind):
    """A bucket of kind "f32", "f16" (np.float16) or "bf16" (np.uint16 bit patterns) as fp32, exactly."""
    if kind == "bf16":
        return bf16_to_f32(x)
    return np.ascontiguousarray(x).astype(F32)


def round_out(a, kind):
    """The fp32 aggregate rounded once to the out dtype."""
    a = np.ascontiguousarray(a, F32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16)
    if kind == "bf16":
        return f32_to_bf16(a)
    return a.copy()


def sumsq(x, g):
    """Rule 1, exactly rounded: x and g fp32 arrays; d = fl32(x - g), the squares exact in fp64, one rounding."""
    with np.errstate(all="ignore"):
        d = (np.ascontiguousarray(x, F32) - np.ascontiguousarray(g, F32)).astype(F32)
        q = d.astype(F64) * d.astype(F64)
    if np.isnan(q).any():
        return float("nan")
    return math.fsum(q.tolist())  # inf terms give inf


def sumsq_bound(n, exact):
    """fa.h: whatever the order, |Q - exact| <= n * 2^-53 * exact."""
    return n * 2.0 ** -53 * exact


def scale(Q, C):
    """Rule 2: (s as np.float32, included)."""
    Q, C = float(Q), float(F32(C))
    N = float("nan") if Q != Q or Q < 0 else math.sqrt(Q)
    if N != N or N == math.inf:
        return F32(0.0), False
    if N <= C:
        return F32(1.0), True
    return F32(C / N), True  # np.float32(python float) rounds to nearest-even


def weights(w, scales, included):
    """Rule 3: (the included clients in ascending order, their fp32 weights w', c0 as np.float32)."""
    W = Wp = 0.0
    inc, wp = [], []
    for k in range(len(w)):
        W += float(F32(w[k]))
        if not included[k]:
            continue
        p = F32(F32(w[k]) * F32(scales[k]))
        Wp += float(p)
        inc.append(k)
        wp.append(p)
    return inc, np.asarray(wp, F32), F32(W - Wp)


def first_term(c0, g):
    """fl32(fma(c0, g, +0)): the product of two fp32 values is exact in fp64, rounded once; -0 becomes +0."""
    with np.errstate(all="ignore"):
        t = (F64(c0) * np.ascontiguousarray(g, F32).astype(F64)).astype(F32)
        return (t + F32(0.0)).astype(F32)


def aggregate(O, xs, kind, w, scales, included, g):
    """Rule 4: the part's fp32 aggregate.  xs: the D receipts of `kind`; g: the fp32 reference."""
    inc, wp, c0 = weights(w, scales, included)
    init = first_term(c0, g) if c0 != 0 else None
    if not inc:
        return init if init is not None else np.zeros(xs[0].size, F32)
    if kind == "bf16":
        return O.fedavg([np.ascontiguousarray(xs[k]) for k in inc], wp, init=init, out_dtype="f32")
    return O.fedavg([widen(xs[k], kind) for k in inc], wp, init=init)


def clip_round(O, xs, kind, w, g, C, Q=None):
    """One clipped round from the squared distances Q (default: the exact ones): (Q, scales, included,
    n_clipped, the fp32 aggregate).  An excluded client has scale 0."""
    if Q is None:
        Q = [sumsq(widen(x, kind), g) for x in xs]
    sc = [scale(q, C) for q in Q]
    scales = np.asarray([s for s, _ in sc], F32)
    included = np.asarray([i for _, i in sc], bool)
    n_clipped = int(sum(1 for s, i in sc if i and s < 1))
    return np.asarray(Q, F64), scales, included, n_clipped, aggregate(O, xs, kind, w, scales, included, g)
