"""GPU: the geomed stage's fused Weiszfeld pass (fa_geomed_pass_device, fa.h "Geomed stage" rule 1) against
tests/geomed_ref.py.

One call gives three things, each checked on its own terms:
(a) v, the chain held in registers, stored on request: bit-equal to fa_reduce_device over the same pointers and
    weights into an f32 output, and to the oracle's chain;
(b) Q_k: the summation order is free, so every Q_k is within n * 2^-53 * exact of the exactly rounded sum of the
    squares of fl32(x_k - v) taken against those v bits (NaN and inf must come back as NaN and inf);
(c) B_k, the count of non-finite inputs: exact.
The client counts sit on every side of every padded width P of the kernel (2, 4, ... 128: 16-byte loads up to 32, the
8-byte form at 64, the 4-byte form at 128), the sizes cover a lone element, less than a vector, less than a tile,
several tiles with head and tail, and ~100 workgroups; the pointer phases select the vector form with and without a
head, and the element form.  The lattice inputs make (a) and (b) exact in closed form for every D from 1 to 128, so
they are compared with no tolerance at all.
"""
import math

import numpy as np
import pytest

import geomed_ref as G
from guarded import GuardedBuf

pytestmark = pytest.mark.gpu

F16, F32, F64, U16 = np.float16, np.float32, np.float64, np.uint16
SEED = 0x6E0D
NS = [1, 7, 67, 4099, 100003]
DS = [1, 2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 128]
KINDS = ["f32", "bf16", "f16"]
ITEM = {"f32": 4, "bf16": 2, "f16": 2}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def bits64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def make_clients(n, D, kind, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, n).astype(F32)
    return [G.round_out((g + F32(0.05 * (1 + k % 7)) * rng.uniform(-1, 1, n).astype(F32)).astype(F32), kind) for k in range(D)]


def place(torch, xs, kind, offsets):
    """The receipts in one device allocation, client k at 16-byte phase offsets[k] (in elements): (keep-alive, ptrs)."""
    item, nbytes = ITEM[kind], np.asarray(xs[0]).size * ITEM[kind]
    stride = (nbytes + 15) // 16 * 16 + 16
    pool = torch.zeros(len(xs) * stride + 16, dtype=torch.uint8, device="cuda")
    base = pool.data_ptr()
    first = (-base) % 16
    ptrs = []
    for k, x in enumerate(xs):
        start = first + k * stride + offsets[k] * item
        pool[start:start + nbytes].copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)))
        ptrs.append(base + start)
    torch.cuda.synchronize()
    return pool, ptrs


def v_buffer(torch, n, kind, offsets):
    """A guarded fp32 buffer for v whose phase lets the vector form run when the clients share one."""
    V = 16 // ITEM[kind]
    head = (-offsets[0]) % V
    return GuardedBuf(torch, n * 4, (-4 * head) % 16 if len(set(offsets)) == 1 else 0)


def check_q(q, exact, n, what):
    for k in range(len(exact)):
        if exact[k] != exact[k]:
            assert q[k] != q[k], (what, k, q[k])
        elif exact[k] == math.inf:
            assert q[k] == math.inf, (what, k, q[k])
        else:
            err, tol = abs(float(q[k]) - exact[k]), G.sumsq_bound(n, exact[k])
            assert err <= tol, "%s: Q[%d] = %r, exact %r, error %g > bound %g" % (what, k, q[k], exact[k], err, tol)


def run_pass(fa, torch, xs, kind, w, offsets, ref, what, ctx=None):
    """One call at the given phases, checked against ref = (v, Q exact, B); returns the Q bits."""
    n, D = np.asarray(xs[0]).size, len(xs)
    vref, qref, bref = ref
    pool, ptrs = place(torch, xs, kind, offsets)
    vb = v_buffer(torch, n, kind, offsets)
    q, b = fa.geomed_pass_device(ptrs, w, n, fa_dt(fa, kind), v=vb.ptr, ctx=ctx)
    vb.check(what)
    v = vb.view(torch.float32).cpu().numpy()
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    fa.reduce_device(ptrs, w, n, fa_dt(fa, kind), out, fa.F32, fa.FEDAVG, ctx=ctx)
    torch.cuda.synchronize()
    G.assert_bits(v, out.cpu().numpy(), what + ": v against fa_reduce_device")
    G.assert_bits(v, vref, what + ": v against the oracle chain")
    check_q(q, qref, n, what)
    assert b.tolist() == bref.tolist(), (what, b, bref)
    q2, b2 = fa.geomed_pass_device(ptrs, w, n, fa_dt(fa, kind), ctx=ctx)  # as the stage calls it: v not stored
    assert np.array_equal(bits64(q2), bits64(q)) and b2.tolist() == b.tolist(), what + ": without v_out"
    del pool
    return bits64(q)


# ------------------------------------------------------------------ sizes, client counts, dtypes, phases

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_fused_pass_over_sizes_and_phases(fa, O, torch_gpu, D, kind):
    w = O.weights(D)
    V = 16 // ITEM[kind]
    for n in NS:
        xs = make_clients(n, D, kind, SEED + 13 * n + D)
        ref = G.fused_pass(O, xs, kind, w)
        assert not ref[2].any()
        for offsets in ([0] * D, [1] * D, [k % V for k in range(D)] if D > 1 else [V - 1]):
            run_pass(fa, torch_gpu, xs, kind, w, offsets, ref, "%s D %d n %d phases %s" % (kind, D, n, offsets[:4]))


def test_strided_tiles_and_determinism(fa, O, torch_gpu):
    """A grid capped below the tile count (98 tiles of 1024 elements on 3 workgroups), and the same call twice."""
    n, D = 100003, 8
    xs = make_clients(n, D, "f32", SEED + 4)
    w = O.weights(D)
    ref = G.fused_pass(O, xs, "f32", w)
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=3)
        run_pass(fa, torch_gpu, xs, "f32", w, [0] * D, ref, "3 workgroups", ctx=agg)
        run_pass(fa, torch_gpu, xs, "f32", w, [0, 1, 2, 3, 0, 1, 2, 3], ref, "3 workgroups, element form", ctx=agg)
    a = run_pass(fa, torch_gpu, xs, "f32", w, [0] * D, ref, "one-shot grid")
    b = run_pass(fa, torch_gpu, xs, "f32", w, [0] * D, ref, "one-shot grid again")
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ lattice inputs: no tolerance
#
# x_k[i] = scale c_k u_i with c_k = k + 1, u_i in {-2, -1, 1, 2} and one power-of-two weight 2^-s for everyone, so
#     v_i = scale u_i S,  S = D (D + 1) / 2^(s+1),   Q_k = scale^2 (c_k - S)^2 sum_i u_i^2
# and every product, partial sum of the chain, difference, square and partial sum of any order is an integer times a
# power of two that fits its format (|c u| <= 256 is exact in bf16; the chain's numerators stay below 2^15, the
# differences' below 2^17, the sums below 2^53).  With s = 8, 2 S = D (D + 1) / 256 is never an integer for D <= 128
# (one of D, D + 1 is odd and the other below 256), so no two clients lie at the same distance from v: a sum routed
# to the wrong client shows.

LATTICE_N = 4121


def lattice(kind, scale_exp):
    u = np.asarray([-2, -1, 1, 2], np.int64)[np.random.default_rng(SEED).integers(0, 4, LATTICE_N)]
    xs = []
    for k in range(128):
        val = np.ldexp(((k + 1) * u).astype(F64), scale_exp)
        x = G.round_out(val.astype(F32), kind)
        assert np.array_equal(G.widen(x, kind).astype(F64), val), "client %d of the lattice is not exact in %s" % (k, kind)
        xs.append(x)
    return u, xs


def lattice_expected(u, D, s, scale_exp):
    su = int((u * u).sum())
    num_s, den = D * (D + 1), 2 ** (s + 1)  # S = num_s / den
    v = np.ldexp((u * num_s).astype(F64), scale_exp - (s + 1)).astype(F32)
    assert np.array_equal(v.astype(F64), np.ldexp((u * num_s).astype(F64), scale_exp - (s + 1)))
    q = []
    for k in range(D):
        num = (den * (k + 1) - num_s) ** 2 * su
        assert num < 2 ** 53
        q.append(math.ldexp(float(num), 2 * scale_exp - 2 * (s + 1)))
    return v, np.asarray(q, F64)


def run_lattice(fa, torch, kind, Ds, s, scale_exp, offsets_of):
    u, xs = lattice(kind, scale_exp)
    for phase in offsets_of:
        pool, ptrs = place(torch, xs, kind, [phase(k) for k in range(128)])
        vb = v_buffer(torch, LATTICE_N, kind, [phase(k) for k in range(128)])
        for D in Ds:
            w = np.full(D, 2.0 ** -s, F32)
            q, b = fa.geomed_pass_device(ptrs[:D], w, LATTICE_N, fa_dt(fa, kind), v=vb.ptr)
            v, qx = lattice_expected(u, D, s, scale_exp)
            what = "%s lattice D %d phase %d scale 2^%d" % (kind, D, phase(1), scale_exp)
            G.assert_bits(vb.view(torch.float32).cpu().numpy(), v, what + ": v")
            assert np.array_equal(bits64(q), bits64(qx)), (what, q, qx)
            assert not b.any(), (what, b)
            assert len(set(qx.tolist())) == D or s != 8, what
        vb.check(kind + " lattice")
        del pool


@pytest.mark.parametrize("kind", KINDS)
def test_lattice_every_client_count_bit_for_bit(fa, torch_gpu, kind):
    V = 16 // ITEM[kind]
    run_lattice(fa, torch_gpu, kind, range(1, 129), 8, 0, [lambda k: 1, lambda k: k % V])


@pytest.mark.parametrize("kind", KINDS)
def test_lattice_at_the_smallest_subnormal_is_not_flushed(fa, torch_gpu, kind):
    """Inputs, v and every difference are subnormal in fp32 (f32: all of them; 16-bit types: in their own format)."""
    e = {"f32": -149, "bf16": -133, "f16": -24}[kind]
    run_lattice(fa, torch_gpu, kind, range(1, 129), 0, e, [lambda k: 1])


# ------------------------------------------------------------------ planted elements

PLANT_N = 5000  # at phase 1: a head of 3, four whole tiles of 1024 and one of 900, a tail of 1
PLANT_AT = {"head": 1, "first tile": 103, "last partial tile": 4599, "tail": 4999}


@pytest.mark.parametrize("where", sorted(PLANT_AT))
@pytest.mark.parametrize("what", ["overflow", "nan", "inf"])
def test_planted_elements(fa, O, torch_gpu, what, where):
    D, i = 3, PLANT_AT[where]
    xs = make_clients(PLANT_N, D, "f32", SEED + 5)
    w = np.asarray([0.25, 0.5, 0.25], F32)
    if what == "overflow":  # 3e38 against a v near -1.5e38: the fp32 difference overflows, nothing is non-finite
        xs[0][i], xs[1][i], xs[2][i] = 3e38, -3e38, -3e38
    elif what == "nan":
        xs[1][i] = np.nan
    else:
        xs[2][i] = -np.inf
    ref = G.fused_pass(O, xs, "f32", w)
    run_pass(fa, torch_gpu, xs, "f32", w, [1] * D, ref, "%s in the %s" % (what, where))
    vref, qref, bref = ref
    if what == "overflow":
        assert qref[0] == math.inf and np.isfinite(qref[1:]).all() and not bref.any() and np.isfinite(vref).all()
    elif what == "nan":
        assert bref.tolist() == [0, 1, 0] and np.isnan(qref).all()
    else:
        assert bref.tolist() == [0, 0, 1] and np.isnan(qref[2]) and (qref[:2] == math.inf).all()


def test_non_finite_counts_add_up_across_lanes_waves_and_workgroups(fa, O, torch_gpu):
    n, D = 100003, 5
    xs = make_clients(n, D, "bf16", SEED + 6)
    rng = np.random.default_rng(SEED)
    counts = [0, 1, 700, 64, 4099]
    for k, c in enumerate(counts):
        at = rng.choice(n, c, replace=False)
        xs[k][at] = rng.choice(np.asarray([0x7FC0, 0x7F80, 0xFF80], U16), c)  # NaN, +inf, -inf
    w = O.weights(D)
    ref = G.fused_pass(O, xs, "bf16", w)
    assert ref[2].tolist() == counts
    run_pass(fa, torch_gpu, xs, "bf16", w, [0] * D, ref, "bf16 counts, vector form")
    run_pass(fa, torch_gpu, xs, "bf16", w, [0, 1, 2, 3, 4], ref, "bf16 counts, element form")
