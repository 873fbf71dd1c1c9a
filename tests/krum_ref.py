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


# ------------------------------------------------------------------ lattice inputs: rule 1 in closed form
#
# Client k holds x_k[i] = scale * c_k * u_i with small integers u_i and scale a power of two, so
#     Q_ab = scale^2 (c_a - c_b)^2 sum_i u_i^2
# and every difference, square and partial sum in any order is an integer times a power of two that fits its
# format: a kernel that follows rule 1 returns exactly these bits, whatever its summation order.

LATTICE_CLIENTS = 128
LATTICE_SEED = 0x1A77
LATTICE_N = 4121  # the GPU sweep's size (tests/test_krum_geometry_gpu.py asserts what it needs of it)
# the smallest subnormal of each type: x = scale c u is then subnormal in its type (bf16: up to |c u| = 127; the
# larger ones fill the first normal binade) and every fl32 difference below 2^23 steps is an fp32 subnormal
SUBNORMAL_SCALE = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24}
SMALLEST_NORMAL = {"f32": 2.0 ** -126, "bf16": 2.0 ** -126, "f16": 2.0 ** -14}


_MIAN_CHOWLA = {}


def mian_chowla(count):
    """The first `count` terms of the Mian-Chowla sequence (greedy Sidon: all pairwise sums a + b, a <= b, differ,
    hence all positive differences differ, hence all (c_a - c_b)^2 of distinct unordered pairs)."""
    if count not in _MIAN_CHOWLA:
        _MIAN_CHOWLA[count] = _mian_chowla(count)
    return list(_MIAN_CHOWLA[count])


def _mian_chowla(count):
    seq, sums, x = [], set(), 0
    while len(seq) < count:
        x += 1
        new = {x + y for y in seq} | {2 * x}
        if sums.isdisjoint(new):
            seq.append(x)
            sums |= new
    return seq


def pow2_exponent(scale):
    m, e = math.frexp(scale)
    assert m == 0.5, "scale %r is not a power of two" % (scale,)
    return e - 1


def lattice(n, kind, scale=1.0):
    """(c, u, xs): the coefficients of the LATTICE_CLIENTS clients (np.int64), the n integers u_i in {-2 .. 2}
    (np.int64, seeded, never 0: an element that is dropped or taken twice changes every pair's sum) and the
    buckets xs[k] = scale c_k u_i of `kind`.  f32: c is the Mian-Chowla sequence, so every matrix entry names its
    pair; bf16 and f16: c_k = k, so |c_k u_i| <= 254 is exact in both."""
    u = np.asarray([-2, -1, 1, 2], np.int64)[np.random.default_rng(LATTICE_SEED).integers(0, 4, n)]
    c = np.asarray(mian_chowla(LATTICE_CLIENTS) if kind == "f32" else range(LATTICE_CLIENTS), np.int64)
    e = pow2_exponent(scale)
    xs = []
    for k in range(LATTICE_CLIENTS):
        v = np.ldexp((c[k] * u).astype(F64), e)  # exact in fp64
        x = round_out(v.astype(F32), kind)
        assert np.array_equal(widen(x, kind).astype(F64), v), "client %d of the lattice is not exact in %s" % (k, kind)
        xs.append(x)
    return c, u, xs


def lattice_distances(c, u, scale=1.0, D=None):
    """The closed form of rule 1 for the first D lattice clients over the elements u: exact integers (< 2^53,
    asserted) times scale^2."""
    c = [int(v) for v in np.asarray(c)[:D]]
    su = sum(int(v) * int(v) for v in np.asarray(u))
    D = len(c)
    Q = np.zeros((D, D), F64)
    for a in range(D):
        for b in range(a + 1, D):
            q = (c[a] - c[b]) ** 2 * su
            assert q < 2 ** 53
            Q[a, b] = Q[b, a] = math.ldexp(float(q), 2 * pow2_exponent(scale))
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
