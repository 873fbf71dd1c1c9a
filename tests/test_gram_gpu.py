"""GPU: the Gram pass (fa.gram_device, csrc/fa_gram.hip) against the int64 numpy product on lattice inputs.

x_k[i] = scale * c_k[i] with seeded integers |c| <= 15 and scale a power of two, the reference scale * r_i with
integers |r| <= 15: every y = scale (c - r), every product and every partial sum in any order is an exact integer
times scale^2, so the whole matrix -- diagonal and mirror included -- must come back bit for bit, whatever the order
of the kernel's fp64 adds.  Scales: 1, 2^40 and the type's smallest subnormal; fp16 takes 2^11 for 2^40, the largest
power of two at which 15 * scale is still an fp16 number.

Sizes, from the kernel's constants (fa_internal.h gram_tile: a tile holds E = 256, 128, 64, 64, 32, 32, 32, 32 elements
at B = ceil(D / 16) = 1 .. 8 blocks of clients): n = 1, n = E - 1 (one tile minus one element) and n = 3 E + 5 on a
context capped at two workgroups, so that workgroup 0 takes tiles 0 and 2 and the last tile is partial.  At pointer
phase 0 the vector form runs (and the element form its tail); at a shared phase of one element the element form takes
the head and the tail around it; n = 1 is the element form alone.
"""
import numpy as np
import pytest

import dnc_ref as R
from clip_ref import round_out, widen

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DS = [1, 2, 15, 16, 17, 32, 33, 64, 65, 113, 128]
KINDS = ["f32", "bf16", "f16"]
SCALES = {"f32": [0, 40, -149], "bf16": [0, 40, -133], "f16": [0, 11, -24]}  # exponents of the scale


def tile(D):
    return (256, 128, 64, 64, 32, 32, 32, 32)[(D + 15) // 16 - 1]


def bits(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def upload(torch, rows, phase):
    """The rows of a 2-D array on the device, each `phase` elements past a 16-byte boundary: (keep-alive, pointers)."""
    (D, n), item = rows.shape, rows.itemsize
    stride = (n * item + 15) // 16 * 16 + 16
    host = np.zeros(D * stride + 16, np.uint8)
    for k in range(D):
        lo = k * stride + phase * item
        host[lo:lo + n * item] = np.ascontiguousarray(rows[k]).view(np.uint8)
    dev = torch.from_numpy(host).cuda()
    return dev, [dev.data_ptr() + k * stride + phase * item for k in range(D)]


def lattice(D, n, kind, e, with_ref, seed):
    """(the buckets of `kind`, the fp32 reference or None, the expected matrix)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-15, 16, (D, n))
    r = rng.integers(-15, 16, n) if with_ref else np.zeros(n, np.int64)
    xs = np.stack([round_out(np.ldexp(c[k].astype(F64), e).astype(F32), kind) for k in range(D)])
    assert all(np.array_equal(widen(xs[k], kind).astype(F64), np.ldexp(c[k].astype(F64), e)) for k in range(D))
    y = c - r
    G = np.ldexp((y @ y.T).astype(F64), 2 * e)
    return xs, (np.ldexp(r.astype(F64), e).astype(F32) if with_ref else None), G


def run(fa, torch, agg, xs, ref, kind, phase):
    dt = {"f32": fa.F32, "bf16": fa.BF16, "f16": fa.F16}[kind]
    keep, ptrs = upload(torch, xs, phase)
    rkeep, rptr = upload(torch, ref[None, :], phase) if ref is not None else (None, [None])
    return fa.gram_device(ptrs, xs.shape[1], dt, ref=rptr[0], ctx=agg)


@pytest.mark.parametrize("with_ref", [False, True], ids=["plain", "ref"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_lattice_is_bit_exact(fa, torch_gpu, D, kind, with_ref):
    E = tile(D)
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=2)
        for phase in (0, 1):
            for n in (1, E - 1, 3 * E + 5):
                for e in SCALES[kind]:
                    xs, ref, G = lattice(D, n, kind, e, with_ref, 1000 * D + n)
                    got = run(fa, torch_gpu, agg, xs, ref, kind, phase)
                    what = "D %d %s n %d phase %d scale 2^%d" % (D, kind, n, phase, e)
                    assert got.shape == (D, D) and np.array_equal(bits(got), bits(got.T)), what + ": not bit-symmetric"
                    bad = np.argwhere(bits(got) != bits(G))
                    assert not len(bad), "%s: %d entries differ, first G%s = %r, expected %r" % (
                        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], G[tuple(bad[0])])


def test_random_data_is_within_the_derived_bound(fa, torch_gpu):
    """|G_ab - exact| <= n 2^-53 sum_i |y_a,i y_b,i| (fa.h "Gram pass"), exact = math.fsum of the fp64 products."""
    D, n = 33, 4099
    rng = np.random.default_rng(0x6A4)
    xs = rng.standard_normal((D, n)).astype(F32)
    ref = rng.standard_normal(n).astype(F32)
    with fa.Aggregator(1) as agg:
        for r in (None, ref):
            got = run(fa, torch_gpu, agg, xs, r, "f32", 0)
            ys = xs if r is None else (xs - r).astype(F32)
            for a in range(D):
                for b in range(a, D):
                    exact, mass = R.gram_entry(ys[a], ys[b])
                    err, tol = abs(float(got[a, b]) - exact), n * 2.0 ** -53 * mass
                    assert err <= tol and bits(got[a, b]) == bits(got[b, a]), (a, b, got[a, b], exact, err, tol)


@pytest.mark.parametrize("D,p", [(17, 16), (65, 3)])
def test_a_nonfinite_client_reaches_its_row_and_column_only(fa, torch_gpu, D, p):
    """Client p holds an inf in the first tile and a NaN in the tail: row and column p are NaN, the rest the lattice's."""
    n = 3 * tile(D) + 5
    xs, _, G = lattice(D, n, "f32", 0, False, 77)
    xs[p, 5], xs[p, n - 1] = np.inf, np.nan
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=2)
        got = run(fa, torch_gpu, agg, xs, None, "f32", 0)
    assert np.isnan(got[p]).all() and np.isnan(got[:, p]).all(), got[p]
    others = np.delete(np.arange(D), p)
    assert np.array_equal(bits(got[np.ix_(others, others)]), bits(G[np.ix_(others, others)]))
