"""Structured columns for the sorting kernels (fa_trimmed.hip, fa_centered.hip, fa_sortnet.h), with expected
values that need no sort.

Not a test module.  A column is one element: D values, one per client.  Three kinds:

* two-valued ("0-1") columns: z clients hold `lo`, D - z hold `hi`.  A comparator network sorts every input iff
  it sorts every 0-1 input, and the trimmed mean of such a column has the closed form `closed_form`: the window
  [t, D - t) holds n_lo = clamp(z - t, 0, D - 2t) lows.  The families are boolean masks (D, C), True = low:
  `exhaustive` (all 2^D), `few` (at most two lows or two highs at every pair of positions), `thresholds`
  ([pi(k) < z] for every z of a permutation pi) and `wide_split` (every split (z0, z1) of the lows between
  clients 0..63 and 64..D-1: every path of the wide form's merge);
* `permutations`: the clients hold 0..D-1 in a random order, small integers whose sums are exact;
* `slide_columns`: j far lows and theta - j equal values, on which the centred mean's window starts exactly at
  min(j, theta - keep).

Every value is exact in fp32, bf16 and fp16.  tests/test_trimmed_cpu.py and tests/test_bulyan_cpu.py prove the
closed form and the window starts against trimmed_ref / bulyan_ref; tests/test_sort_forms_gpu.py runs the
columns through the kernels.
"""
import numpy as np

import trimmed_ref as T

F32 = np.float32

# (lo, hi) of the two-valued columns.  "nan": a NaN key equals the pad key, so pads mix with NaNs.
PAIRS01 = {"01": (0.0, 1.0), "pm1": (-1.0, 1.0), "nan": (1.0, np.nan)}

DS_EXHAUSTIVE = list(range(1, 17))      # every pattern: the compiled networks of P = 2 .. 16, pads included
DS_NETWORK = [23, 32, 47, 64]           # P = 32 and 64, full and with pads
DS_WIDE = [65, 66, 96, 127, 128]        # the wide form: a second half of 1, 2, 32, 63 and 64 clients
SLIDE_THETAS = [7, 16, 23, 32, 47, 64, 65, 100, 128]
SEED = 0x50C7


def trim_set(D):
    """The ends, the quarter and the two last trims of D, then the median by its own name."""
    top = (D - 1) // 2
    return sorted({t for t in (0, 1, 2, (D - 1) // 4, top - 1, top) if 0 <= t and 2 * t < D}) + [T.TRIM_MEDIAN]


def trims_for(D):
    """The trims the structured columns run at D: every one up to D = 16, trim_set above."""
    return list(range((D - 1) // 2 + 1)) + [T.TRIM_MEDIAN] if D <= 16 else trim_set(D)


def keeps_for(theta):
    """The keeps the 0-1 families run through the centred mean: every one up to theta = 8, then the ends, the
    quarters and both sides of the middle."""
    if theta <= 8:
        return list(range(1, theta + 1))
    ks = (1, 2, 3, theta // 4, theta // 2, theta // 2 + 1, 3 * theta // 4, theta - 2, theta - 1, theta)
    return sorted({k for k in ks if 1 <= k <= theta})


# ------------------------------------------------------------------ two-valued columns

def closed_form(D, trim, z, pair):
    """The fp32 trimmed mean of columns with z lows (an integer array) of PAIRS01[pair], without a sort."""
    t = T.resolve(trim, D)
    m = D - 2 * t
    assert 0 <= t and m > 0
    n_lo = np.clip(np.asarray(z, np.int64) - t, 0, m)
    n_hi = m - n_lo
    if pair == "01":
        return (n_hi.astype(F32) / F32(m)).astype(F32)
    if pair == "pm1":  # the partial sums are integers of magnitude <= D: exact, and -k + k = +0
        return ((n_hi - n_lo).astype(F32) / F32(m)).astype(F32)
    assert pair == "nan"
    return np.where(n_hi > 0, F32(np.nan), F32(1.0)).astype(F32)


def values(mask, pair):
    """(D, C) fp32 values of a mask: lo where True."""
    lo, hi = PAIRS01[pair]
    return np.where(mask, F32(lo), F32(hi)).astype(F32)


def exhaustive(D):
    c = np.arange(1 << D, dtype=np.int64)
    return ((c[None, :] >> np.arange(D, dtype=np.int64)[:, None]) & 1).astype(bool)


def few(D):
    """Every column with 0, 1 or 2 lows, then every column with 0, 1 or 2 highs."""
    a, b = np.triu_indices(D, 1)
    two = np.zeros((D, a.size), bool)
    two[a, np.arange(a.size)] = True
    two[b, np.arange(a.size)] = True
    lows = np.concatenate([np.zeros((D, 1), bool), np.eye(D, dtype=bool), two], axis=1)
    return np.concatenate([lows, ~lows], axis=1)


def permutations(D, R, seed=SEED):
    """(D, R) int64: R random permutations of 0..D-1, one per column."""
    rng = np.random.default_rng(seed + 7 * D)
    return np.stack([rng.permutation(D) for _ in range(R)], axis=1).astype(np.int64)


def thresholds(perms):
    """[pi(k) < z] for every permutation (column of perms) and z = 0..D."""
    D, R = perms.shape
    z = np.arange(D + 1, dtype=np.int64)
    return (perms[:, :, None] < z[None, None, :]).reshape(D, R * (D + 1))


def wide_split(D, seed=SEED):
    """One column per (z0, z1), z0 = 0..64 lows among clients 0..63 and z1 = 0..D-64 among clients 64..D-1,
    at random places inside each half."""
    assert 64 < D <= 128
    rng = np.random.default_rng(seed + 11 * D)
    z0, z1 = np.meshgrid(np.arange(65), np.arange(D - 64 + 1), indexing="ij")
    z0, z1 = z0.ravel(), z1.ravel()
    r0 = np.argsort(np.argsort(rng.random((64, z0.size)), axis=0), axis=0)
    r1 = np.argsort(np.argsort(rng.random((D - 64, z0.size)), axis=0), axis=0)
    return np.concatenate([r0 < z0[None, :], r1 < z1[None, :]], axis=0)


def n_perms(D):
    """R of the threshold family: about a thousand columns per D."""
    return max(8, 1024 // (D + 1))


def families(D):
    """[(name, mask)] of the two-valued families run at D."""
    if D in DS_EXHAUSTIVE:
        return [("exhaustive", exhaustive(D))]
    if D <= 64:
        return [("few", few(D)), ("thresholds", thresholds(permutations(D, n_perms(D))))]
    return [("wide split", wide_split(D)), ("thresholds", thresholds(permutations(D, n_perms(D))))]


def zero_one(D):
    """All two-valued columns of D side by side, padded with all-high columns to an odd count that is no
    multiple of a 16-byte vector: (mask (D, C), z (C,))."""
    mask = np.concatenate([m for _, m in families(D)], axis=1)
    pad = (3 - mask.shape[1]) % 8
    mask = np.concatenate([mask, np.zeros((D, pad), bool)], axis=1)
    return mask, mask.sum(axis=0)


def perm_values(D, R=64):
    """(D, R) fp32: the permutations themselves as values."""
    return permutations(D, R, SEED + 1).astype(F32)


# ------------------------------------------------------------------ slide columns of the centred mean

def slide_targets(theta, keep):
    """The window starts rule 4 can reach on the slide columns."""
    return list(range(min(theta - keep, (theta - 1) // 2) + 1))


def slide_columns(theta, copies=2, seed=SEED):
    """(x (theta, C) fp32, target (C,)): for every j = 0..(theta-1)//2, `copies` columns with the j distinct far
    lows -(1024 + 8 u) and theta - j values 1.0, scattered over the clients.  While the window's lowest value is
    a far low, the lower difference is positive and the upper one is not, so it slides; once it is 1.0 both
    differences are 0 and it stops: the start is min(j, theta - keep).  -(1024 + 8 u), u < 64, is exact in bf16."""
    rng = np.random.default_rng(seed + 13 * theta)
    cols, target = [], []
    for j in range((theta - 1) // 2 + 1):
        v = np.ones(theta, F32)
        v[:j] = -(1024.0 + 8.0 * np.arange(j))
        for _ in range(copies):
            cols.append(rng.permutation(v))
            target.append(j)
    return np.stack(cols, axis=1).astype(F32), np.asarray(target, np.int64)
