"""The secagg stage's rule (fa.h "Secagg stage") in numpy: ChaCha20 block words, the unmasked sum, the decode."""
import numpy as np

U32, U64, F32 = np.uint32, np.uint64, np.float32
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"
QUARTERS = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
            (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def _rotl(x, n):
    return (x << U32(n)) | (x >> U32(32 - n))


def block_words(key, nonce, counters):
    """The 16 output words of the RFC 8439 2.3 block function for every block counter: uint32[len(counters), 16]."""
    counters = np.asarray(counters, U64)
    init = [np.full(counters.size, w, U32) for w in SIGMA] + [np.full(counters.size, int(w), U32) for w in key]
    init += [counters.astype(U32)] + [np.full(counters.size, int(w), U32) for w in nonce]
    x = [w.copy() for w in init]
    with np.errstate(over="ignore"):
        for _ in range(10):
            for a, b, c, d in QUARTERS:
                x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
                x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
                x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
                x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)
        return np.stack([x[j] + init[j] for j in range(16)], axis=1)


def mask(key, nonce, idx0, n):
    """Rule 2: the mask words of bucket elements idx0 .. idx0 + n - 1."""
    if n == 0:
        return np.empty(0, U32)
    b0, b1 = idx0 >> 4, (idx0 + n - 1) >> 4
    words = block_words(key, nonce, np.arange(b0, b1 + 1, dtype=U64)).reshape(-1)
    return words[idx0 - 16 * b0: idx0 - 16 * b0 + n].copy()


def unmask(ys, keys, nonces, signs, idx0=0):
    """Rule 3: the sum modulo 2^32 of the buckets ys and the signed mask words."""
    u = np.zeros(len(ys[0]), U32)
    with np.errstate(over="ignore"):
        for y in ys:
            u += np.asarray(y).view(U32)
        for key, nonce, sign in zip(keys, nonces, signs):
            m = mask(key, nonce, idx0, u.size)
            u = u + m if sign > 0 else u - m
    return u


def decode(u, scale):
    """Rule 4: fl32((float)(int32)u * scale)."""
    return (u.view(np.int32).astype(F32) * F32(scale)).astype(F32)
