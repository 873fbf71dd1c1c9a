"""The noise stage of fa.h ("Noise stage") in numpy: uint32 / uint64 integer operations and float32 operations only.

No numpy operation fuses a multiply with an add, float32 division and square root are correctly rounded, and
subnormals are kept, so every function here gives the bits the rule specifies.  `normals` is the reference of
fa_noise_host and of the kernel; `apply` is rule 4; `exact` is the same transform in float64 from the same
uniforms and angles (the accuracy condition's yardstick).
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

f32 = np.float32
SQRT2 = f32(math.sqrt(2.0))
LN2 = f32(math.log(2.0))
PI4 = f32(math.pi / 4.0)
C3, C5, C7, C9 = f32(1.0 / 3.0), f32(1.0 / 5.0), f32(1.0 / 7.0), f32(1.0 / 9.0)
S3, S5, S7, S9 = f32(-1.0 / 6.0), f32(1.0 / 120.0), f32(-1.0 / 5040.0), f32(1.0 / 362880.0)
K2, K4, K6, K8 = f32(-1.0 / 2.0), f32(1.0 / 24.0), f32(-1.0 / 720.0), f32(1.0 / 40320.0)
TWO_M23 = f32(2.0 ** -23)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & MASK


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0..c3) and key (k0, k1); arrays or scalars of 32-bit words -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(_u32(c)) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _uniform_parts(r):
    """Rule 2's (mant, b) of N = r + 1: the top 24 bits of N with bit b at bit 23, and b itself."""
    N = np.asarray(r, dtype=np.uint64) + np.uint64(1)
    b = (np.frexp(N.astype(np.float64))[1] - 1).astype(np.int64)  # exact: N < 2^53
    down = np.maximum(b - 23, 0).astype(np.uint64)
    up = np.maximum(23 - b, 0).astype(np.uint64)
    mant = (N >> down) << up
    return mant, b


def radius(r):
    """Rule 2: R = sqrt(-2 ln u) of the word r, float32."""
    mant, b = _uniform_parts(r)
    m = mant.astype(np.float32) * TWO_M23
    e = (b - 32).astype(np.int32)
    big = m > SQRT2
    m = np.where(big, m * f32(0.5), m).astype(np.float32)
    e = np.where(big, e + 1, e).astype(np.int32)
    f = m - f32(1.0)
    s = f / (f32(2.0) + f)
    t = s * s
    p = C9 * t
    p = p + C7
    p = p * t
    p = p + C5
    p = p * t
    p = p + C3
    p = p * t
    p = p * s
    p = p + s
    l = p + p
    L = e.astype(np.float32) * LN2 + l
    assert L.dtype == np.float32
    return np.sqrt(f32(-2.0) * L)


def direction(r):
    """Rule 3: (cos, sin) of the angle q pi/2 + x of the word r, float32."""
    r = np.asarray(r, dtype=np.uint32)
    q = r >> np.uint32(30)
    k = (r & np.uint32(0x3FFFFFFF)) >> np.uint32(6)
    v = (k.astype(np.int32) - np.int32(1 << 23)).astype(np.float32) * TWO_M23
    x = v * PI4
    y = x * x
    p = S9 * y
    p = p + S7
    p = p * y
    p = p + S5
    p = p * y
    p = p + S3
    p = p * y
    p = p * x
    sx = p + x
    p = K8 * y
    p = p + K6
    p = p * y
    p = p + K4
    p = p * y
    p = p + K2
    p = p * y
    cx = p + f32(1.0)
    assert cx.dtype == np.float32 and sx.dtype == np.float32
    co = np.where(q == 0, cx, np.where(q == 1, -sx, np.where(q == 2, -cx, sx)))
    si = np.where(q == 0, sx, np.where(q == 1, cx, np.where(q == 2, -sx, -cx)))
    return co.astype(np.float32), si.astype(np.float32)


def pair(ra, rb):
    """Rule 4's two normals of the word pair (ra: radius, rb: direction)."""
    R = radius(ra)
    c, s = direction(rb)
    return R * c, R * s


def exact_pair(ra, rb):
    """The same transform in float64 from the same uniform u and angle."""
    mant, b = _uniform_parts(ra)
    u = np.ldexp(mant.astype(np.float64), (b - 23 - 32).astype(np.int64))
    rb = np.asarray(rb, dtype=np.uint32)
    q = (rb >> np.uint32(30)).astype(np.float64)
    k = ((rb & np.uint32(0x3FFFFFFF)) >> np.uint32(6)).astype(np.float64)
    v = (k - 2.0 ** 23) * 2.0 ** -23
    ang = v * (math.pi / 4.0) + q * (math.pi / 2.0)
    R = np.sqrt(-2.0 * np.log(u))
    return R * np.cos(ang), R * np.sin(ang)


def split_seed(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def group_words(seed, stream, rnd, j):
    """The four Philox words of groups j (uint64 array)."""
    j = np.asarray(j, dtype=np.uint64)
    k0, k1 = split_seed(seed)
    return philox4x32_10(j & MASK, j >> np.uint64(32), np.uint64(rnd), np.uint64(stream), k0, k1)


def group_normals(seed, stream, rnd, j):
    """[len(j), 4] float32: the normals of elements 4j .. 4j+3."""
    r0, r1, r2, r3 = group_words(seed, stream, rnd, j)
    z0, z1 = pair(r0, r1)
    z2, z3 = pair(r2, r3)
    return np.stack([z0, z1, z2, z3], axis=1).astype(np.float32)


def normals(seed, stream, rnd, idx0, n):
    """The n unit normals of elements idx0 .. idx0 + n - 1 of the bucket (float32)."""
    if n == 0:
        return np.zeros(0, np.float32)
    j0, j1 = idx0 >> 2, (idx0 + n - 1) >> 2
    z = group_normals(seed, stream, rnd, np.arange(j0, j1 + 1, dtype=np.uint64)).reshape(-1)
    lo = idx0 - 4 * j0
    return np.ascontiguousarray(z[lo:lo + n])


def apply(a, stddev, z):
    """Rule 4: a' = fl(a + fl(stddev * z)), float32."""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (a + f32(stddev) * z.astype(np.float32)).astype(np.float32)


def noisy(a, stddev, seed, stream, rnd, idx0=0):
    return apply(a, stddev, normals(seed, stream, rnd, idx0, len(a)))
