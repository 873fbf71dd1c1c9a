"""numpy restatement of low-rank receipts (include/fedavg/fa.h, "Low-rank receipts"): length, decode and expansion.

Not a test module.  It follows the rule, not the library: an fp64 matmul per matrix, one rounding to fp32, numpy's fp32
add, the slot rounding of mx8_ref.  A table is a list of (off, rows, cols).  The test bucket holds every edge shape of
the kernel's 64 x 64 tiles and 16 x 16 blocks, with rest gaps before, between and after the matrices and the matrix
offsets at every 4-byte phase modulo 16 bytes.
"""
import numpy as np

from mx8_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
SHAPES = [(1, 1), (15, 17), (16, 16), (65, 63), (130, 7), (7, 130)]
GAPS = [3, 5, 2, 2, 7, 4, 6]  # rest elements before each matrix, and after the last


def bucket():
    """(table, n): SHAPES laid out with GAPS between them."""
    mats, off = [], 0
    for (rows, cols), gap in zip(SHAPES, GAPS):
        mats.append((off + gap, rows, cols))
        off += gap + rows * cols
    assert sorted({m[0] % 4 for m in mats}) == [0, 1, 2, 3]
    return mats, off + GAPS[-1]


def rest_mask(mats, n):
    rest = np.ones(n, bool)
    for off, rows, cols in mats:
        rest[off:off + rows * cols] = False
    return rest


def length(mats, n, r):
    return r * sum(rows + cols for _, rows, cols in mats) + int(rest_mask(mats, n).sum())


def factors(f, mats, r):
    """[(P, Q)] as views of f, and the rest values."""
    out, at = [], 0
    for _, rows, cols in mats:
        out.append((f[at:at + rows * r].reshape(rows, r), f[at + rows * r:at + (rows + cols) * r].reshape(cols, r)))
        at += (rows + cols) * r
    return out, f[at:]


def lattice(mats, n, r, seed):
    """A receipt whose every fp64 sum and fp32 rounding is exact whatever the order: factor entries are integers in
    [-8, 8] times one power of two per matrix; the rest is random."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(length(mats, n, r)).astype(F32)
    for j, (P, Q) in enumerate(factors(f, mats, r)[0]):
        P[:] = rng.integers(-8, 9, P.shape) * F32(2.0) ** (j - 3)
        Q[:] = rng.integers(-8, 9, Q.shape) * F32(2.0) ** (2 - j)
    return f


def sums(f, mats, n, r):
    """(S in fp64 for the covered elements and the rest values elsewhere, sum_t |p q| in fp64, 0 for rest)."""
    pq, rest = factors(np.asarray(f, F32), mats, r)
    S, A = np.zeros(n, np.float64), np.zeros(n, np.float64)
    S[rest_mask(mats, n)] = rest
    with np.errstate(all="ignore"):
        for (off, rows, cols), (P, Q) in zip(mats, pq):
            P, Q = P.astype(np.float64), Q.astype(np.float64)
            S[off:off + rows * cols] = (P @ Q.T).reshape(-1)
            A[off:off + rows * cols] = (np.abs(P) @ np.abs(Q).T).reshape(-1)
    return S, A


def decode(f, mats, n, r):
    with np.errstate(all="ignore"):
        return sums(f, mats, n, r)[0].astype(F32)


def expand(f, mats, n, r, idx0, cnt, slot_kind, g=None, ref_kind="f32"):
    """The slot (of slot_kind) over bucket elements [idx0, idx0 + cnt) from the receipt and the reference g of that
    range (of ref_kind; None: absolute)."""
    d = decode(f, mats, n, r)[idx0:idx0 + cnt]
    if g is None:
        return round_out(d, slot_kind)
    with np.errstate(all="ignore"):
        return round_out((widen(g, ref_kind) + d).astype(F32), slot_kind)
