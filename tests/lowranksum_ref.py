"""The low-rank-sum stage (include/fedavg/fa.h, "Low-rank-sum stage", rules 1-4) restated in plain numpy.

Not a test module.  It follows the rule, not the library: one fp32 multiply of P by the weight, an fp64 matmul per owner and
matrix added owner by owner, one rounding to fp32; the exact fmaf chain of sparse_ref on the rest; numpy's fp32 add of the
widened reference.  Receipts, tables and the test bucket are those of lowrank_ref.
"""
import numpy as np

import lowrank_ref as L
from lowrank_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)
from sparse_ref import fmaf

F32, F64 = np.float32, np.float64


def sums(fs, rs, w, mats, n):
    """(S, A): on a matrix the stacked sum of rule 2 and sum |p' q|, both in fp64; on the rest the chain of rule 3 and 0."""
    S, A, rest = np.zeros(n, F64), np.zeros(n, F64), L.rest_mask(mats, n)
    acc = np.zeros(int(rest.sum()), F32)
    with np.errstate(all="ignore"):
        for f, r, wc in zip(fs, rs, w):
            pq, rv = L.factors(np.asarray(f, F32), mats, r)
            for (off, rows, cols), (P, Q) in zip(mats, pq):
                P, Q = (F32(wc) * P).astype(F32).astype(F64), Q.astype(F64)  # rule 1, then exact widening
                S[off:off + rows * cols] += (P @ Q.T).reshape(-1)
                A[off:off + rows * cols] += (np.abs(P) @ np.abs(Q).T).reshape(-1)
            acc = fmaf(F32(wc), rv, acc)
    S[rest] = acc
    return S, A


def lowrank_sum(fs, rs, w, mats, n, g=None):
    """a fp32[n] over the whole bucket; g: the widened reference, or None (absolute mode)."""
    with np.errstate(all="ignore"):
        acc = sums(fs, rs, w, mats, n)[0].astype(F32)
        return acc if g is None else (np.ascontiguousarray(g, F32) + acc).astype(F32)


def assert_exact(fs, rs, w, mats, n):
    """Lattice receipts (lowrank_ref.lattice) under weights from {1/8 .. 8/8}: rule 1 is exact and every partial sum, in
    any order, is an integer below 2^24 times 2^-4 -- so every order of the fp64 adds and the one rounding give the same
    bits."""
    for f, r, wc in zip(fs, rs, w):
        for P, _ in L.factors(np.asarray(f, F32), mats, r)[0]:
            assert np.array_equal((F32(wc) * P).astype(F64), F64(wc) * P.astype(F64))
    A = sums(fs, rs, w, mats, n)[1] * 16
    assert np.array_equal(A, np.rint(A)) and A.max() < 2 ** 24
