"""The MX8-sum stage (fa.h "MX8-sum stage", rules 1-3) restated in plain numpy: mx8_ref.decode per client, the exact fmaf
of sparse_ref for the chain, one fp32 add against the widened reference.  The tests compare libfa's host function and its
kernels against this, every bit."""
import numpy as np

from mx8_ref import E_EDGES, IDX0S, assert_bits, decode, round_out, widen  # noqa: F401  (re-exported for the tests)
from sparse_ref import fmaf

F32 = np.float32
Q_EDGES = np.array([-128, -127, -1, 0, 1, 127], np.int8)


def mx8_sum(q, e, w, idx0=0, g=None):
    """a fp32[n] over bucket elements idx0 ..: rules 1-2 client by client, then rule 3 against g, the widened reference, or
    None."""
    acc = np.zeros(len(q[0]), F32)
    for c in range(len(q)):
        acc = fmaf(F32(w[c]), decode(q[c], e[c], idx0), acc)
    if g is None:
        return acc
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(g, F32) + acc).astype(F32)


def receipts(D, n, idx0, seed, edges=True):
    """D receipts over bucket elements idx0 .. idx0 + n - 1: random codes with the edge codes sprinkled in, every block's E
    drawn from E_EDGES (edges) or from ordinary scales."""
    rng = np.random.default_rng(seed)
    nb = ((idx0 + n - 1) >> 5) - (idx0 >> 5) + 1
    q = [rng.integers(-127, 128, n).astype(np.int8) for _ in range(D)]
    for x in q:
        x[::3] = rng.choice(Q_EDGES, x[::3].size)
    e = [(rng.choice(E_EDGES, nb) if edges else rng.integers(120, 140, nb)).astype(np.uint8) for _ in range(D)]
    return q, e
