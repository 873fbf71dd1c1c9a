"""The sign-vote stage (fa.h "Sign-vote stage") restated in plain numpy: int64 counts, np.float32 arithmetic with one
operation per line, the vote planes.  The tests compare libfa's host function and its kernels against this, every bit."""
import numpy as np

from mx8_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)

F32, U32 = np.float32, np.uint32
MAJORITY, MEAN = 0, 1


def words(n):
    return (n + 31) // 32


def pack(delta):
    """Rule 2: the bit of element i is set iff delta_i < 0 (clear for -0 and NaN); padding bits 0."""
    delta = np.ascontiguousarray(delta, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        b = np.zeros(words(delta.size) * 32, np.uint8)
        b[:delta.size] = delta < 0
    return np.packbits(b, bitorder="little").view(U32).copy()


def unpack(bits, idx0, n):
    """Elements idx0 .. idx0 + n - 1 of a whole receipt as 0 / 1."""
    return np.unpackbits(np.ascontiguousarray(bits, U32).view(np.uint8), bitorder="little")[idx0:idx0 + n].astype(np.int64)


def to_plane(flags):
    b = np.zeros(words(flags.size) * 32, np.uint8)
    b[:flags.size] = flags
    return np.packbits(b, bitorder="little").view(U32).copy()


def vote(bits, n, eta, rule=MAJORITY, margin=1, g=None, idx0=0):
    """(a fp32[n], neg, pos): rules 3-9 over the whole receipts `bits`; g: the widened reference (fp32[n]) or None; the
    planes are None under the mean rule."""
    D = len(bits)
    c = np.zeros(n, np.int64)
    for b in bits:
        c += unpack(b, idx0, n)
    s = D - 2 * c
    eta = F32(eta)
    neg = pos = None
    if rule == MAJORITY:
        v = np.where(s >= margin, 1, np.where(-s >= margin, -1, 0))
        t = np.where(v > 0, eta, np.where(v < 0, -eta, F32(0))).astype(F32)
        neg, pos = to_plane(v < 0), to_plane(v > 0)
    else:
        step = F32(eta / F32(D))
        sf = s.astype(F32)
        t = (sf * step).astype(F32)
    if g is None:
        return t, neg, pos
    with np.errstate(all="ignore"):
        a = (np.ascontiguousarray(g, F32) + t).astype(F32)
    return a, neg, pos


def receipts(D, n, seed):
    """D whole receipts of n elements whose per-element bias makes the counts reach 0, D and everything between."""
    rng = np.random.default_rng(seed)
    bias = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], n)
    return [to_plane(rng.random(n) < bias) for _ in range(D)]
