"""numpy restatement of rot1 receipts (include/fedavg/fa.h, "Rot1 receipts").  Not a test module.  It follows the rule,
not the library: W is the butterfly loop in float32, the sum of |y| the pairwise tree in float64, the diagonal comes
from noise_ref.philox4x32_10.  bf16 values travel as ``np.uint16`` bit patterns, fp16 as ``np.float16``."""
import numpy as np

import noise_ref
from mx8_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)

F32, F64, U32 = np.float32, np.float64, np.uint32
B, WORDS = 4096, 128
STREAM = 0x524F5431
QNAN = np.asarray([0x7FC00000], U32).view(F32)[0]


def blocks(n):
    return (n + B - 1) // B


def signs(seed, blk0, nb):
    """s_i of the elements of blocks blk0 .. blk0 + nb - 1, as bools [nb, 4096]."""
    j = np.arange(blk0 * 32, (blk0 + nb) * 32, dtype=np.uint64)
    r = noise_ref.philox4x32_10(j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), 0, STREAM, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(r, axis=1).reshape(-1)  # group j: words 4 j .. 4 j + 3
    return ((words[:, None] >> np.arange(32, dtype=U32)) & U32(1)).astype(bool).reshape(nb, B)


def flip(x, s):
    return (np.ascontiguousarray(x, F32).view(U32) ^ (s.astype(U32) << U32(31))).view(F32)


def transform(z):
    """W on the rows of z [nb, 4096], float32, h = 1 .. 2048."""
    z = np.array(z, F32)
    h = 1
    with np.errstate(all="ignore"):
        while h < B:
            v = z.reshape(z.shape[0], B // (2 * h), 2, h)
            a, b = v[:, :, 0, :].copy(), v[:, :, 1, :].copy()
            v[:, :, 0, :], v[:, :, 1, :] = a + b, a - b
            h *= 2
    return z


def unpack(bits, nb):
    w = np.ascontiguousarray(bits, U32)[:nb * WORDS]
    return ((w[:, None] >> np.arange(32, dtype=U32)) & U32(1)).astype(bool).reshape(nb, B)


def decode(bits, scale, seed, idx0, cnt):
    """Rules 1-4: the deltas of bucket elements [idx0, idx0 + cnt); bits and scale start at block idx0 >> 12."""
    blk0 = idx0 >> 12
    nb = ((idx0 + cnt - 1) >> 12) - blk0 + 1
    v = transform(np.where(unpack(bits, nb), F32(-1), F32(1)))
    with np.errstate(all="ignore"):
        d = flip((v * np.ascontiguousarray(scale, F32)[:nb, None]).astype(F32), signs(seed, blk0, nb)).reshape(-1)
    lo = idx0 - blk0 * B
    return d[lo:lo + cnt].copy()


def expand(bits, scale, seed, idx0, cnt, slot_kind, g=None, ref_kind="f32"):
    """The slot (of slot_kind) from the receipt and the reference g (of ref_kind; None: absolute)."""
    d = decode(bits, scale, seed, idx0, cnt)
    if g is None:
        return round_out(d, slot_kind)
    with np.errstate(all="ignore"):
        return round_out((widen(g, ref_kind) + d).astype(F32), slot_kind)


def encode_delta(delta, seed):
    """Rules 2-5 on the deltas of a whole bucket: (bits uint32[128 nb], scale float32[nb])."""
    delta = np.ascontiguousarray(delta, F32).reshape(-1)
    nb = blocks(delta.size)
    pad = np.zeros(nb * B, F32)
    pad[:delta.size] = delta
    y = transform(flip(pad, signs(seed, 0, nb).reshape(-1)).reshape(nb, B))
    with np.errstate(all="ignore"):
        a = np.abs(y).astype(F64)
        while a.shape[1] > 1:
            a = a[:, 0::2] + a[:, 1::2]
        A = a[:, 0]
        bad = ~(A < np.inf)
        scale = np.where(bad, QNAN, (A * 2.0 ** -24).astype(F32)).astype(F32)
        neg = (y < 0) & ~bad[:, None]
    bits = (neg.reshape(-1, 32).astype(U32) << np.arange(32, dtype=U32)).sum(axis=1, dtype=U32)
    return bits, scale


def encode(new, sent, kind, seed):
    """Rules 1-6 on `new` and `sent` of one kind: (bits, scale, g')."""
    with np.errstate(all="ignore"):
        delta = (widen(new, kind) - widen(sent, kind)).astype(F32)
    bits, scale = encode_delta(delta, seed)
    return bits, scale, expand(bits, scale, seed, 0, delta.size, kind, sent, kind)
