"""CPU: the noise stage's rule (fa.h "Noise stage") -- tests/noise_ref.py against the known answers, the accuracy
condition and the distribution bounds, and fa_noise_host (the kernel's own source, compiled for the host) against
noise_ref bit for bit.  No GPU: fa_noise_device is only probed (n == 0) and refused.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import noise_ref as N
from conftest import PKG_DIR

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
UNIT = 2.0 ** -24
DIST_SEED = 0x0000567800001234  # key words 0x1234, 0x5678
DIST_ROUND, DIST_STREAM, DIST_GROUPS = 7, 0, 1 << 22


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def scatter(count, mul=2654435761, add=0):
    """A multiplicative scatter of `count` 32-bit words."""
    return ((np.arange(count, dtype=U64) * U64(mul) + U64(add)) & U64(0xFFFFFFFF)).astype(U32)


@pytest.fixture(scope="module")
def dist_words():
    return N.group_words(DIST_SEED, DIST_STREAM, DIST_ROUND, np.arange(DIST_GROUPS, dtype=U64))


@pytest.fixture(scope="module")
def dist_normals(dist_words):
    r0, r1, r2, r3 = dist_words
    z0, z1 = N.pair(r0, r1)
    z2, z3 = N.pair(r2, r3)
    return np.stack([z0, z1, z2, z3], axis=1).reshape(-1)


# ------------------------------------------------------------------ rule 1

def test_philox_known_answers():
    cases = [
        ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, want in cases:
        got = " ".join("%08x" % int(w[0]) for w in N.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, key, got)


def test_counter_and_key_layout():
    """Group j, round, stream and the seed's halves sit where fa.h puts them."""
    seed, stream, rnd, j = 0xA4093822_299F31D0 >> 0, 0x03707344, 0x13198A2E, (0x85A308D3 << 32) | 0x243F6A88
    k0, k1 = N.split_seed(seed)
    assert (k0, k1) == (0x299F31D0, 0xA4093822)
    got = N.group_words(seed, stream, rnd, np.asarray([j], U64))
    want = N.philox4x32_10(0x243F6A88, 0x85A308D3, rnd, stream, k0, k1)
    assert [int(a[0]) for a in got] == [int(a[0]) for a in want]


# ------------------------------------------------------------------ rules 2-4: edges and accuracy

def test_radius_edges():
    R = N.radius(np.asarray([0xFFFFFFFF, 0, 0xFFFFFFFE, 0x7FFFFFFF], U32))
    assert bits(R)[0] == 0x80000000  # N = 2^32: u = 1, R = -0
    assert abs(float(R[1]) - math.sqrt(-2.0 * math.log(2.0 ** -32))) < 1e-5 and float(R[1]) < 6.6605
    assert 0 < float(R[2]) < 4e-4  # u = 1 - 2^-24
    assert abs(float(R[3]) - math.sqrt(2.0 * math.log(2.0))) < 1e-6  # u = 1/2
    z0, z1 = N.pair(np.asarray([0xFFFFFFFF] * 4, U32), np.asarray([0, 1 << 30, 2 << 30, 3 << 30], U32))
    assert not (bits(z0) & 0x7FFFFFFF).any() and not (bits(z1) & 0x7FFFFFFF).any()  # both normals are zeros


def test_direction_quadrants():
    words = np.asarray([(q << 30) | (1 << 29) for q in range(4)], U32)  # x = 0 in every quadrant
    c, s = N.direction(words)
    assert c.tolist() == [1.0, -0.0, -1.0, 0.0] and s.tolist() == [0.0, 1.0, -0.0, -1.0]
    c, s = N.direction(scatter(1 << 16))
    assert np.abs(c.astype(F64) ** 2 + s.astype(F64) ** 2 - 1).max() < 4 * UNIT


def worst_units(ra, rb):
    z0, z1 = N.pair(ra, rb)
    e0, e1 = N.exact_pair(ra, rb)
    worst = 0.0
    for z, e in ((z0, e0), (z1, e1)):
        worst = max(worst, float((np.abs(z.astype(F64) - e) / (UNIT * np.maximum(1.0, np.abs(e)))).max()))
    return worst


def test_accuracy_condition(dist_words):
    """Every normal within 8 * 2^-24 * max(1, |z|) of the fp64 transform of the same u and angle: 2^22 groups
    (2^24 normals) and the edge sets.  Measured: 4.05 units on the groups, 3.83 on the edge sets."""
    r0, r1, r2, r3 = dist_words
    figures = {"groups (r0, r1)": worst_units(r0, r1), "groups (r2, r3)": worst_units(r2, r3)}
    low = np.arange(65536, dtype=U32)
    high = (U32(0xFFFFFFFF) - low).astype(U32)
    # direction edges: the ends and the middle of every quadrant's 24-bit range, with every low-bit pattern
    k = np.asarray([0, 1, 2, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1], U32)
    dir_edges = np.asarray([(q << 30) | (int(kk) << 6) | low6 for q in range(4) for kk in k for low6 in (0, 63)], U32)
    for name, ra in (("r0 in 0..65535", low), ("the top 65536", high), ("scatter", scatter(1 << 20, add=977))):
        for mul in (2654435761, 40503):
            figures["%s x scatter %d" % (name, mul)] = worst_units(ra, scatter(ra.size, mul, 12345))
        reps = -(-ra.size // dir_edges.size)
        figures["%s x direction edges" % name] = worst_units(ra, np.tile(dir_edges, reps)[:ra.size])
    for name, v in figures.items():
        print("%-40s %.3f units" % (name, v))
    assert max(figures.values()) <= 8.0, figures


def test_distribution(dist_normals):
    z = dist_normals
    n = z.size
    assert n == 1 << 24 and np.isfinite(z).all() and float(np.abs(z).max()) <= 6.6605
    zd = z.astype(F64)
    mean, var = float(zd.mean()), float(zd.var())
    import torch
    s = torch.sort(torch.from_numpy(zd)).values
    cdf = (0.5 * (1.0 + torch.erf(s / math.sqrt(2.0)))).numpy()
    i = np.arange(1, n + 1, dtype=F64)
    ks = float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()))
    print("mean %.3e var %.6f KS %.3e" % (mean, var, ks))
    assert abs(mean) <= 4.0 / math.sqrt(n)
    assert abs(var - 1.0) <= 4.0 * math.sqrt(2.0 / n)
    assert ks <= 1.63 / math.sqrt(n)


def test_streams_rounds_and_seeds_differ():
    j = np.arange(64, dtype=U64)
    base = N.group_normals(DIST_SEED, 0, 0, j)
    for seed, stream, rnd in ((DIST_SEED, 1, 0), (DIST_SEED, 0, 1), (DIST_SEED + 1, 0, 0), (DIST_SEED + (1 << 32), 0, 0)):
        other = N.group_normals(seed, stream, rnd, j)
        assert (bits(other) != bits(base)).mean() > 0.99


# ------------------------------------------------------------------ the host twin

@pytest.mark.parametrize("idx0", [0, 1, 2, 3, 2 ** 34 - 6])
def test_noise_host_equals_the_reference(fa, idx0):
    for n in (1, 7, 67, 4099):
        for seed, stream, rnd in ((DIST_SEED, 0, 7), (0xFEDCBA9876543210, 0xFFFFFFFF, 0xFFFFFFFF), (0, 3, 0)):
            got = fa.noise_host(seed, stream, rnd, idx0, n)
            want = N.normals(seed, stream, rnd, idx0, n)
            assert got.dtype == F32 and np.array_equal(bits(got), bits(want)), (idx0, n, seed)


def test_noise_host_over_the_distribution_run(fa, dist_normals):
    got = fa.noise_host(DIST_SEED, DIST_STREAM, DIST_ROUND, 0, dist_normals.size)
    assert np.array_equal(bits(got), bits(dist_normals))


def test_noise_host_is_cut_anywhere(fa):
    whole = fa.noise_host(5, 6, 7, 2 ** 32 - 11, 41)
    for cut in (1, 2, 3, 4, 5, 17, 40):
        a = fa.noise_host(5, 6, 7, 2 ** 32 - 11, cut)
        b = fa.noise_host(5, 6, 7, 2 ** 32 - 11 + cut, 41 - cut)
        assert np.array_equal(bits(np.concatenate([a, b])), bits(whole))
    assert fa.noise_host(5, 6, 7, 0, 0).size == 0


# ------------------------------------------------------------------ the probe and the refusals without a context

def test_device_entry_probe_touches_no_device(fa):
    for dt in (fa.F32, fa.BF16, fa.F16):
        fa.noise_device(None, 0, None, dt, stddev=1.0, seed=1, stream_id=2, round=3, idx0=2 ** 40)


def test_refusals_without_a_context(fa):
    def refused(code, word, **kw):
        args = dict(avg=None, n=0, out=None, out_dtype=fa.F32, stddev=1.0, seed=1)
        args.update(kw)
        with pytest.raises(fa.FaError) as e:
            fa.noise_device(**args)
        assert e.value.code == code and word in str(e.value), str(e.value)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(fa.ERR_ARG, "stddev", stddev=bad)
    refused(fa.ERR_ARG, "dtype", out_dtype=7)
    refused(fa.ERR_ARG, "2^64", n=16, idx0=2 ** 64 - 8, avg=64, out=64)
    refused(fa.ERR_ARG, "d_avg", n=4, out=64)
    refused(fa.ERR_ARG, "d_out", n=4, avg=64)
    refused(fa.ERR_ALIGN, "aggregate", n=4, avg=66, out=64)
    refused(fa.ERR_ALIGN, "output", n=4, avg=64, out=66)
    refused(fa.ERR_ALIGN, "output", n=4, avg=64, out=65, out_dtype=fa.BF16)
    L = fa.lib()
    assert L.fa_set_noise(None, -1, 1.0, 1) == fa.ERR_ARG and "ctx" in fa.last_error()
    assert L.fa_set_noise(None, -1, float("nan"), 1) == fa.ERR_ARG and "stddev" in fa.last_error()
    assert L.fa_set_noise(None, -1, -0.5, 1) == fa.ERR_ARG and "stddev" in fa.last_error()
    assert L.fa_get_noise(None, -1, None, None) == fa.ERR_ARG
    r = ctypes.c_uint64()
    assert L.fa_noise_get_round(None, 0, ctypes.byref(r)) == fa.ERR_ARG
    assert L.fa_noise_set_round(None, 0, 0) == fa.ERR_ARG
    assert L.fa_noise_host(1, 0, 0, 0, 4, None) == fa.ERR_ARG and "z is null" in fa.last_error()
    assert L.fa_noise_host(1, 0, 0, 2 ** 64 - 2, 4, None) == fa.ERR_ARG and "2^64" in fa.last_error()


# ------------------------------------------------------------------ the drop-in's flags

def test_flag_refusals():
    AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR

    def refused(flags, word):
        r = subprocess.run([AGG, "-i", "-1", "-d", "3", "-c", "1"] + flags, capture_output=True, text=True, timeout=30)
        assert r.returncode == 2 and word in r.stderr.splitlines()[0], r.stderr[:300]

    refused(["--dp-noise-multiplier", "1"], "needs --clip-norm")
    refused(["--dp-seed", "1", "--clip-norm", "1"], "--dp-seed goes with")
    refused(["--dp-noise-multiplier", "1", "--clip-norm", "1", "--mode", "literal"], "--mode literal")
    refused(["--dp-noise-multiplier", "1", "--clip-norm", "1", "--layout", "rs"], "--layout rs")
    refused(["--dp-noise-multiplier", "0", "--clip-norm", "1"], "finite and > 0")
    refused(["--dp-noise-multiplier", "nan", "--clip-norm", "1"], "finite and > 0")
