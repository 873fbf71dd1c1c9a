"""numpy restatement of the Krum stage (include/fedavg/fa.h, "Krum stage"): the expected values of the Krum tests.

Not a test module.  Rule 1 is computed exactly (``math.fsum`` of the fp64 squares of the fl32 differences: the
stage's own summation order is free, so the tests bound its error instead of fixing it); rules 2-4 are plain
fp64 / fp32 arithmetic; rule 5 is the oracle's ordered FMA chain ``O.fedavg`` over the selected clients.  bf16
values travel as ``np.uint16`` bit patterns.
"""
import math

import numpy as np

from clip_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64


def pair_sumsq(x, y):
    """Rule 1 for one pair, exactly rounded: x and y fp32 arrays; d = fl32(x - y), the squares exact in fp64, one
    rounding.  A NaN term gives NaN, an inf term inf."""
    with np.errstate(all="ignore"):
        d = (np.ascontiguousarray(x, F32) - np.ascontiguousarray(y, F32)).astype(F32)
        q = d.astype(F64) * d.astype(F64)
    if np.isnan(q).any():
        return float("nan")
    return math.fsum(q.tolist())  # inf terms give inf


def distances(xs, kind):
    """Rule 1: the D x D matrix of the receipts `xs` of `kind`; each pair once and mirrored, the diagonal +0."""
    ws = [widen(x, kind) for x in xs]
    D = len(ws)
    Q = np.zeros((D, D), F64)
    for a in range(D):
        for b in range(a + 1, D):
            Q[a, b] = Q[b, a] = pair_sumsq(ws[a], ws[b])
    return Q


def dist_bound(n, exact):
    """fa.h: whatever the order, |Q - exact| <= n * 2^-53 * exact."""
    return n * 2.0 ** -53 * exact


def scores(Q, f):
    """Rule 2: S_k = the D - f - 2 smallest of Q_kj, j != k (NaN as +inf), added ascending from +0."""
    Q = np.asarray(Q, F64)
    D = Q.shape[0]
    S = np.empty(D, F64)
    for k in range(D):
        row = [float(Q[k, j]) for j in range(D) if j != k]
        row = sorted(math.inf if v != v else v for v in row)
        acc = 0.0
        for v in row[:D - f - 2]:
            acc = acc + v
        S[k] = acc
    return S


def select(S, m):
    """Rule 3: the flags of the first m clients by (S_k, k) ascending; S_k = +inf is never selected."""
    D = len(S)
    order = sorted(range(D), key=lambda k: (math.inf if S[k] != S[k] else float(S[k]), k))
    sel = np.zeros(D, bool)
    for k in order[:m]:
        if not float(S[k]) < math.inf:
            break
        sel[k] = True
    return sel


def krum_select(Q, f, m=None):
    """Rules 2-3: (scores, selected); m None: D - f."""
    D = np.asarray(Q).shape[0]
    S = scores(Q, f)
    return S, select(S, D - f if m is None else m)


def weights(w, selected):
    """Rule 4: the fp32 weights w' of all D clients (the deselected ones do not enter the chain)."""
    w = np.asarray(w, F32)
    W = Ws = 0.0
    for k in range(len(w)):
        W += float(w[k])
        if selected[k]:
            Ws += float(w[k])
    if all(selected) or not Ws > 0.0:
        return w.copy()
    ratio = W / Ws
    if not math.isfinite(ratio):
        return w.copy()
    with np.errstate(over="ignore"):
        return np.asarray([F32(float(w[k]) * ratio) for k in range(len(w))], F32)


def aggregate(O, xs, kind, w, selected):
    """Rules 4-5: the part's fp32 aggregate under the selection `selected`."""
    wp = weights(w, selected)
    inc = [k for k in range(len(xs)) if selected[k]]
    if not inc:
        return np.zeros(np.asarray(xs[0]).size, F32)
    if kind == "bf16":
        return O.fedavg([np.ascontiguousarray(xs[k]) for k in inc], wp[inc], out_dtype="f32")
    return O.fedavg([widen(xs[k], kind) for k in inc], wp[inc])


def krum_round(O, xs, kind, w, f, m=None, Q=None):
    """One round from the matrix Q (default: the exact one): (Q, scores, selected, the fp32 aggregate)."""
    if Q is None:
        Q = distances(xs, kind)
    S, sel = krum_select(Q, f, m)
    return np.asarray(Q, F64), S, sel, aggregate(O, xs, kind, w, sel)
