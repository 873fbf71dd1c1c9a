"""numpy restatement of the geomed stage (include/fedavg/fa.h, "Geomed stage"): the expected values of the geomed
tests.

Not a test module.  The chain v of rule 1 is the oracle's ordered FMA chain ``O.fedavg``; the sums Q are computed
exactly (``math.fsum`` of the fp64 squares of the fl32 differences: the stage's own summation order is free, so the
tests bound its error instead of fixing it); rules 3-4 are plain fp64 / fp32 arithmetic; rule 5 is the oracle's chain
again.  bf16 values travel as ``np.uint16`` bit patterns.
"""
import math

import numpy as np

from clip_ref import assert_bits, round_out, sumsq, sumsq_bound, widen  # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64
MAX_ITERS, MAX_CLIENTS = 64, 128


def chain(O, xs, kind, w):
    """The FA_FEDAVG chain of the receipts `xs` of `kind` under the fp32 weights w, into fp32; +0 without clients."""
    if not len(xs):
        raise ValueError("the chain needs a client")
    w = np.ascontiguousarray(w, F32)
    if kind == "bf16":
        return O.fedavg([np.ascontiguousarray(x) for x in xs], w, out_dtype="f32")
    return O.fedavg([widen(x, kind) for x in xs], w)


def nonfinite(xs, kind):
    """B_k of rule 1: the count of NaN / inf elements of every bucket."""
    return np.asarray([int((~np.isfinite(widen(x, kind))).sum()) for x in xs], F64)


def fused_pass(O, xs, kind, w):
    """Rule 1 over all the clients given: (v fp32, Q exactly rounded float64[D], B float64[D])."""
    v = chain(O, xs, kind, w)
    Q = np.asarray([sumsq(widen(x, kind), v) for x in xs], F64)
    return v, Q, nonfinite(xs, kind)


def weights(w, Q, included, nu):
    """Rules 3-4: (alpha float32[D], included bool[D], objective).  W is the fp64 sum of every w_k > 0 in client
    order; a client whose w_k is not > 0, or whose sqrt(Q_k) is NaN or inf, leaves `included` and gets weight 0."""
    w = np.asarray(w, F32)
    D = len(w)
    inc = [bool(i) for i in included]
    nu = float(F32(nu))
    W = B = obj = 0.0
    beta = [0.0] * D
    for k in range(D):
        if not float(w[k]) > 0.0:
            inc[k] = False
            continue
        W += float(w[k])
        if not inc[k]:
            continue
        q = float(Q[k])
        N = float("nan") if q != q or q < 0 else math.sqrt(q)
        if N != N or N == math.inf:
            inc[k] = False
            continue
        obj += float(w[k]) * N
        beta[k] = float(w[k]) / max(nu, N)
        B += beta[k]
    plain = not B > 0.0
    if not plain:
        with np.errstate(all="ignore"):
            ratio = float(F64(W) / F64(B))  # an overflow is inf, inf / inf is NaN: both fall back to w
        plain = not math.isfinite(ratio)
    out = np.zeros(D, F32)
    with np.errstate(over="ignore"):
        for k in range(D):
            if inc[k]:
                out[k] = w[k] if plain else F32(beta[k] * ratio)
    return out, np.asarray(inc, bool), obj


def geomed_round(O, xs, kind, w, iters, nu, exact_q=None):
    """Rules 0-5 with exactly rounded sums: a dict with the trace -- sumsq [P, D], weights [P + 1, D], included [D],
    objective [P], passes P, voided (how many passes were void) -- and the fp32 aggregate."""
    w = np.asarray(w, F32)
    D = len(xs)
    n = np.asarray(xs[0]).size
    inc = np.asarray([float(w[k]) > 0.0 for k in range(D)], bool)
    alpha = np.where(inc, w, F32(0)).astype(F32)
    B = nonfinite(xs, kind)
    rows_q, rows_w, objs = [], [], []
    last_q, voided, t = None, 0, 0
    while t < iters:
        idx = [k for k in range(D) if inc[k]]
        if not idx:
            break
        if any(B[k] > 0 for k in idx):  # rule 2: the pass is void
            voided += 1
            for k in idx:
                if B[k] > 0:
                    inc[k] = False
            alpha = np.where(inc, w, F32(0)).astype(F32)
            if last_q is not None:
                alpha, inc, _ = weights(w, last_q, inc, nu)
            continue
        v = chain(O, [xs[k] for k in idx], kind, alpha[idx])
        q = np.zeros(D, F64)
        for k in idx:
            q[k] = sumsq(widen(xs[k], kind), v)
        rows_q.append(q)
        rows_w.append(alpha.copy())
        alpha, inc, obj = weights(w, q, inc, nu)
        objs.append(obj)
        last_q = q
        t += 1
    alpha = np.where(inc, alpha, F32(0)).astype(F32)
    rows_w.append(alpha.copy())
    idx = [k for k in range(D) if inc[k]]
    a = chain(O, [xs[k] for k in idx], kind, alpha[idx]) if idx else np.zeros(n, F32)
    return dict(sumsq=np.asarray(rows_q, F64).reshape(len(rows_q), D), weights=np.asarray(rows_w, F32), included=inc,
                objective=np.asarray(objs, F64), passes=t, voided=voided, aggregate=a)


def aggregate_from_trace(O, xs, kind, wrows, included):
    """Rule 5 from a reported trace: the chain under the last row of weights over the included clients."""
    idx = [k for k in range(len(xs)) if included[k]]
    if not idx:
        return np.zeros(np.asarray(xs[0]).size, F32)
    return chain(O, [xs[k] for k in idx], kind, np.asarray(wrows[-1], F32)[idx])


def check_trace(O, xs, kind, w, nu, trace, what):
    """A reported trace (sumsq, weights, included, objective) against the rules: every Q^t within the bound of the
    exactly rounded sum against v^t rebuilt from the reported alpha^t; alpha^{t+1}, the flags and the objective
    bit-equal to rules 3-4 applied to the reported Q^t.  Returns the fp32 aggregate of rule 5 under the last row."""
    q, wr, included, obj = trace
    D, n = len(xs), np.asarray(xs[0]).size
    P = q.shape[0]
    assert wr.shape == (P + 1, D) and obj.shape == (P,), (what, q.shape, wr.shape, obj.shape)
    inc = np.asarray([float(F32(w[k])) > 0.0 and not (~np.isfinite(widen(xs[k], kind))).any() for k in range(D)], bool)
    for t in range(P):
        idx = [k for k in range(D) if inc[k]]
        assert all(wr[t][k] == 0 for k in range(D) if not inc[k]), (what, t, wr[t], inc)
        v = chain(O, [xs[k] for k in idx], kind, wr[t][idx])
        for k in range(D):
            if not inc[k]:
                assert q[t, k] == 0.0, (what, t, k, q[t, k])
                continue
            exact = sumsq(widen(xs[k], kind), v)
            if exact != exact:
                assert q[t, k] != q[t, k], (what, t, k, q[t, k])
            elif exact == math.inf:
                assert q[t, k] == math.inf, (what, t, k, q[t, k])
            else:
                err, tol = abs(float(q[t, k]) - exact), sumsq_bound(n, exact)
                assert err <= tol, "%s: Q^%d[%d] = %r, exact %r, error %g > bound %g" % (what, t, k, q[t, k], exact, err, tol)
        alpha, inc, o = weights(w, q[t], inc, nu)
        assert_bits(wr[t + 1], alpha, "%s: alpha^%d" % (what, t + 1))
        assert np.float64(o).view(np.uint64) == obj[t:t + 1].view(np.uint64)[0], (what, t, o, obj[t])
    assert included.tolist() == inc.tolist(), (what, included, inc)
    return aggregate_from_trace(O, xs, kind, wr, inc)
