"""numpy restatement of the Bulyan stage (include/fedavg/fa.h, "Bulyan stage"): the expected values of the
Bulyan tests.

Not a test module.  Rule 1 is krum_ref.distances (exactly rounded; the stage's own summation order is free, so
the tests bound its error); rule 2 is plain fp64 arithmetic, written as the rule says it (every row sorted anew
in every round); rules 3-4 follow fa.h literally on the keys of trimmed_ref, vectorised over the elements.
bf16 values travel as ``np.uint16`` bit patterns.
"""
import math

import numpy as np

from krum_ref import assert_bits, distances, round_out, widen  # noqa: F401  (re-exported for the tests)
from trimmed_ref import keys, unkeys

F32, F64 = np.float32, np.float64


def select(Q, f):
    """Rule 2: (order, pick_scores, selected) -- the picks in pick order, the score of each, the flags."""
    Q = np.asarray(Q, F64)
    D = Q.shape[0]
    R = list(range(D))
    theta = D - 2 * f
    order, ps = [], []
    while len(order) < theta:
        c = max(1, len(R) - f - 2)
        best = None
        for k in R:
            row = sorted(math.inf if v != v else v for v in (float(Q[k, j]) for j in R if j != k))
            acc = 0.0
            for v in row[:min(c, len(R) - 1)]:
                acc = acc + v
            key = (math.inf if acc != acc else acc, k)
            if best is None or key < best:
                best = key
        if not best[0] < math.inf:
            break
        order.append(best[1])
        ps.append(best[0])
        R.remove(best[1])
    sel = np.zeros(D, bool)
    sel[order] = True
    return np.asarray(order, np.intc), np.asarray(ps, F64), sel


def keep_for(n_picked, f):
    """Rule 3."""
    return max(1, n_picked - 2 * f)


def centered_f32(xs, keep):
    """Rule 4.  xs: theta arrays of fp32 (already widened); the fp32 result."""
    theta = len(xs)
    assert 1 <= keep <= theta
    s = unkeys(np.sort(np.stack([keys(x) for x in xs]), axis=0))
    n = s.shape[1]
    col = np.arange(n)
    c_lo, c_hi = s[(theta - 1) // 2], s[theta // 2]
    j = np.zeros(n, np.int64)
    sliding = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(theta - keep):
            jj = np.minimum(j, theta - keep - 1)  # a stopped column reads in range; its result is masked
            d_hi = (s[jj + keep, col] - c_hi).astype(F32)
            d_lo = (c_lo - s[jj, col]).astype(F32)
            sliding &= d_hi < d_lo
            j += sliding
        acc = np.zeros(n, F32)
        for u in range(keep):
            acc = (acc + s[j + u, col]).astype(F32)
        return (acc / F32(keep)).astype(F32), j


def centered(xs, keep, kind="f32", out="f32"):
    """Rule 4 with the widening and the one rounding: xs of `kind`, the result in `out` ("bf16": bit patterns)."""
    r, _ = centered_f32([widen(x, kind) for x in xs], keep)
    return round_out(r, out)


def aggregate(xs, kind, selected, f):
    """Rule 3: the part's fp32 aggregate under the selection `selected`."""
    inc = [k for k in range(len(xs)) if selected[k]]
    if not inc:
        return np.zeros(np.asarray(xs[0]).size, F32)
    r, _ = centered_f32([widen(xs[k], kind) for k in inc], keep_for(len(inc), f))
    return r


def bulyan_round(xs, kind, f, Q=None):
    """One round from the matrix Q (default: the exact one): (Q, order, pick_scores, selected, the aggregate)."""
    if Q is None:
        Q = distances(xs, kind)
    order, ps, sel = select(Q, f)
    return np.asarray(Q, F64), order, ps, sel, aggregate(xs, kind, sel, f)


# ------------------------------------------------------------------ special columns for the kernel tests

def special_columns(theta):
    """Columns (each theta fp32 values, in client order) that exercise rule 4's edges; fewer for a tiny theta."""
    inf, nan = np.inf, np.nan
    tiny = F32(2.0 ** -149)
    cols = []

    def col(vals):
        v = np.resize(np.asarray(vals, F32), theta)
        cols.append(v)

    col([1.0])                                   # all equal: every difference is 0, ties keep the lower window
    col([1.0, 1.0, 2.0, 2.0, 3.0])               # duplicates
    col([0.0, -0.0])                             # signed zeros: -0 sorts below +0, differences are +0
    col([tiny, -tiny, 2 * tiny, 0.0, 3 * tiny])  # subnormal differences are kept
    col([inf, 1.0, 2.0, 3.0, -1.0])              # +inf at the top
    col([-inf, 1.0, 2.0, 3.0, 5.0])              # -inf at the bottom: slid away when the centre is finite
    col([-inf, inf, 0.5, 1.5, 2.5])
    v = np.arange(theta, dtype=F32)
    v[0] = nan
    cols.append(v)                               # one NaN: above the window, never slid into
    v = np.arange(theta, dtype=F32)
    v[: theta // 2 + 1] = nan
    cols.append(v[::-1].copy())                  # more NaNs than half: the centre is NaN, no slide
    col([3e38, -3e38, 1.0, 2.0, -2.0])           # differences that overflow to inf
    col([3e38, -3e38])
    return cols
