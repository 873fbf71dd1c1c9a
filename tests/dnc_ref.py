"""numpy restatement of fa.h "Gram pass" and "DnC stage": the expected values of the DnC tests, not a test module.
A Gram entry is computed exactly (``math.fsum`` of the fp64 products: the pass's summation order is free); rules 2-7 are
Python floats, one rounding per operation, sums in client order from +0; rule 8 is krum_ref's."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def gram_entry(ya, yb):
    """(G_ab exactly rounded, sum_i |y_a,i y_b,i|) of two fp32 arrays; a NaN term gives NaN."""
    with np.errstate(all="ignore"):
        p = np.ascontiguousarray(ya, F32).astype(F64) * np.ascontiguousarray(yb, F32).astype(F64)
    if np.isnan(p).any():
        return float("nan"), float("nan")
    return math.fsum(p.tolist()), math.fsum(np.abs(p).tolist())


def dnc_select(G, drop, iters=32):
    """Rules 2-7: (scores float64[D], selected bool[D]) of the D x D matrix G."""
    G = np.asarray(G, F64)
    D = G.shape[0]
    R = [k for k in range(D) if not (G[k, k] != G[k, k] or G[k, k] == math.inf)]
    r = len(R)
    s = np.full(D, math.inf, F64)
    sel = np.zeros(D, bool)
    if r == 0:
        return s, sel
    g = [[float(G[a, b]) for b in R] for a in R]
    rho, mu = [], 0.0
    for a in range(r):
        acc = 0.0
        for b in range(r):
            acc = acc + g[a][b]
        rho.append(acc / r)
        mu = mu + rho[a]
    mu = mu / r
    C = [[((g[a][b] - rho[a]) - rho[b]) + mu for b in range(r)] for a in range(r)]
    star = 0
    for a in range(1, r):
        if C[a][a] > C[star][star]:
            star = a

    def times_c(u):
        t = []
        for k in range(r):
            acc = 0.0
            for b in range(r):
                acc = acc + C[k][b] * u[b]
            t.append(acc)
        return t

    s[R] = 0.0
    if C[star][star] > 0.0:
        u = [C[b][star] for b in range(r)]
        for _ in range(iters):
            t = times_c(u)
            M = math.nan if any(v != v for v in t) else max(abs(v) for v in t)
            if M != M or M == 0.0 or M == math.inf:
                break
            u = [v / M for v in t]
        t = times_c(u)
        for k in range(r):
            s[R[k]] = t[k] * t[k]
    q = max(0, min(drop - (D - r), r - 1))
    order = sorted(R, key=lambda k: (math.inf if s[k] != s[k] else float(s[k]), k), reverse=True)
    sel[R] = True
    sel[order[:q]] = False
    return s, sel
