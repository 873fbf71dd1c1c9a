"""The rot1-sum stage (fa.h "Rot1-sum stage", rules 0-6) restated in plain numpy, fp32 operations in the stated order; an
fp64 reference from fa.rot1_decode per owner with the derived error bound; receipts with edge scales.  The
tests compare libfa's host function and its kernel against the restatement, every bit."""
import numpy as np

from mx8_ref import assert_bits, round_out, widen  # noqa: F401  (re-exported for the tests)

F32, U32, B = np.float32, np.uint32, 4096
SCALE_EDGES = np.array([np.nan, 0.0, -0.0, -0.37, 1e-41, 2.0 ** 100], F32)


def groups(seed):
    """Rule 0: [(seed, owners ascending)], the groups by their lowest slot."""
    out = {}
    for c, s in enumerate(seed):
        out.setdefault(int(s), []).append(c)
    return list(out.items())


def transform(z):
    """Transform W of Rot1 receipts: h = 1 .. 2048 in order, fl32(a + b) and fl32(a - b)."""
    z, h = z.astype(F32), 1
    while h < B:
        v = z.reshape(-1, 2, h)
        a, b = v[:, 0].copy(), v[:, 1].copy()
        v[:, 0], v[:, 1] = a + b, a - b
        h *= 2
    return z


def flips(fa, seed, blk):
    """Diagonal D of block blk: the decoder on an all-plus receipt gives +-4096 and +-0, whose sign is the flip."""
    return np.signbit(fa.rot1_decode(np.zeros(128, U32), np.ones(1, F32), seed, B, idx0=blk * B))


def unpack(words):
    return np.unpackbits(np.ascontiguousarray(words, U32).view(np.uint8), bitorder="little").astype(bool)


def rot1_sum(fa, bits, scale, seed, w, n, idx0=0, g=None, parts=None):
    """a fp32[n] over bucket elements idx0 ..; bits[c], scale[c] from block idx0 >> 12 on.  parts: a list that receives
    per block (T_G per group, sum_G |d_G| over the block) for the bound."""
    seed = np.broadcast_to(np.asarray(seed, np.uint64), (len(bits),))
    blk0, out = idx0 >> 12, np.empty(n, F32)
    with np.errstate(all="ignore"):
        for k in range(((idx0 + n - 1) >> 12) - blk0 + 1):
            acc, T, absd = np.zeros(B, F32), [], np.zeros(B)
            for s, owners in groups(seed):
                z = np.zeros(B, F32)
                for c in owners:
                    t = F32(w[c]) * F32(scale[c][k])
                    z = z + np.where(unpack(bits[c][128 * k:128 * k + 128]), -t, t).astype(F32)
                v = transform(z)
                d = np.where(flips(fa, s, blk0 + k), -v, v).astype(F32)
                acc = acc + d
                T.append((len(owners), sum(abs(float(w[c]) * float(scale[c][k])) for c in owners)))
                absd += np.abs(d.astype(np.float64))
            if parts is not None:
                parts.append((T, absd))
            lo, hi = max(idx0, (blk0 + k) * B), min(idx0 + n, (blk0 + k + 1) * B)
            out[lo - idx0:hi - idx0] = acc[lo & 4095:(lo & 4095) + hi - lo]
        return out if g is None else (np.ascontiguousarray(g, F32) + out).astype(F32)


def exact(fa, bits, scale, seed, w, n, idx0=0, g=None):
    """sum_c w_c scale_c (D H u_c) + g in fp64: the decoder at scale one gives D H u_c exactly."""
    seed = np.broadcast_to(np.asarray(seed, np.uint64), (len(bits),))
    a = np.zeros(n) if g is None else np.asarray(g, np.float64).copy()
    per = (np.arange(idx0, idx0 + n) >> 12) - (idx0 >> 12)
    for c in range(len(bits)):
        v = fa.rot1_decode(bits[c], np.ones(scale[c].size, F32), int(seed[c]), n, idx0=idx0).astype(np.float64)
        a += float(w[c]) * scale[c].astype(np.float64)[per] * v
    return a


def bound(parts, n, idx0=0, g=None):
    """The derived bound per element: per group 4096 T (m + 13) 2^-24 1.01, then (groups + 1) 2^-24 (sum |d_G| + |g|)."""
    out = np.empty(n)
    for k, (T, absd) in enumerate(parts):
        lo, hi = max(idx0, ((idx0 >> 12) + k) * B), min(idx0 + n, ((idx0 >> 12) + k + 1) * B)
        gg = 0.0 if g is None else np.abs(np.asarray(g, np.float64)[lo - idx0:hi - idx0])
        out[lo - idx0:hi - idx0] = sum(B * t * (m + 13) * 2.0 ** -24 * 1.01 for m, t in T) + \
            (len(T) + 1) * 2.0 ** -24 * (absd[lo & 4095:(lo & 4095) + hi - lo] + gg)
    return out


def receipts(fa, D, n, idx0, rng_seed, seed=7, edges=True, small=1.0):
    """D receipts covering bucket elements idx0 .. idx0 + n - 1 (blocks idx0 >> 12 ..): fa.rot1_encode of seeded deltas; with
    `edges` a block of every third owner takes an edge scale.  Returns (bits, scale, seeds)."""
    rng = np.random.default_rng(rng_seed)
    nb = ((idx0 + n - 1) >> 12) - (idx0 >> 12) + 1
    seeds = np.broadcast_to(np.asarray(seed, np.uint64), (D,)).copy()
    bits, scale = [], []
    for c in range(D):
        b, s = fa.rot1_encode((rng.standard_normal(nb * B) * small).astype(F32), int(seeds[c]))
        if edges and c % 3 == 0:
            s[(c // 3) % nb] = SCALE_EDGES[(c // 3) % SCALE_EDGES.size]
        bits.append(b)
        scale.append(s)
    return bits, scale, seeds
