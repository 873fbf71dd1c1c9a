"""numpy restatement of FA_TRIMMED (include/fedavg/fa.h): the expected values of the trimmed-mean tests.

Not a test module.  Every step follows fa.h literally: widen to fp32, map to the unsigned keys, ``np.sort`` the
keys across the clients, decode, add the kept rows in ascending order with fp32 adds from +0, divide by
D - 2t in fp32, round once to a 16-bit output.  bf16 values travel as ``np.uint16`` bit patterns.
"""
import numpy as np

TRIM_MEDIAN = -1


def keys(x):
    """k(x): 0xFFFFFFFF for NaN, ~bits if the sign bit is set, bits | 0x80000000 otherwise."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    k = np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def unkeys(k):
    """The inverse of keys(); 0xFFFFFFFF decodes to the quiet NaN 0x7FFFFFFF."""
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def bf16_to_f32(h):
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x):
    """Round-to-nearest-even on the bits; a NaN stays a quiet NaN."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r).astype(np.uint16)


def widen(x, bf16=False):
    if bf16:
        return bf16_to_f32(x)
    return np.ascontiguousarray(x).astype(np.float32)  # fp16 widens exactly, subnormals included


def resolve(trim, D):
    return (D - 1) // 2 if trim == TRIM_MEDIAN else trim


def trimmed_f32(xs, trim=TRIM_MEDIAN):
    """xs: D arrays of fp32 (already widened).  The fp32 result of steps 2-4."""
    D = len(xs)
    t = resolve(trim, D)
    assert 0 <= t and 2 * t < D
    s = unkeys(np.sort(np.stack([keys(x) for x in xs]), axis=0))
    acc = np.zeros(s.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for j in range(t, D - t):
            acc = (acc + s[j]).astype(np.float32)
        return (acc / np.float32(D - 2 * t)).astype(np.float32)


def trimmed(xs, trim=TRIM_MEDIAN, in_bf16=False, out="f32"):
    """The whole rule.  out: "f32", "f16" (np.float16) or "bf16" (np.uint16 bit patterns)."""
    r = trimmed_f32([widen(x, in_bf16) for x in xs], trim)
    if out == "f16":
        with np.errstate(over="ignore"):
            return r.astype(np.float16)
    if out == "bf16":
        return f32_to_bf16(r)
    return r


def assert_bits(got, ref, what="", ref_f32=None):
    """Bit for bit over all elements; where the expected value is NaN only a NaN is required."""
    assert got.shape == ref.shape and got.dtype.itemsize == ref.dtype.itemsize, (got.shape, ref.shape, got.dtype)
    ut = np.uint16 if ref.dtype.itemsize == 2 else np.uint32
    g, r = got.view(ut), ref.view(ut)
    if ref.dtype == np.uint16:  # bf16 bit patterns
        rn, gn = np.isnan(bf16_to_f32(r)), np.isnan(bf16_to_f32(g))
    else:
        rn, gn = np.isnan(ref), np.isnan(got.view(ref.dtype))
    assert np.array_equal(gn, rn), "%s: NaN positions differ (%d got, %d expected)" % (what, gn.sum(), rn.sum())
    bad = np.flatnonzero((g != r) & ~rn)
    assert bad.size == 0, "%s: %d/%d mismatches, first at %s: got %s expected %s" % (
        what, bad.size, r.size, bad[:4], g[bad[:4]], r[bad[:4]])
