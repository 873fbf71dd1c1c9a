"""GPU: fp16 buckets (FA_F16) through the C ABI, bit for bit against the oracle.

Expected values need nothing fp16 in the oracle: fp16 inputs are widened exactly with numpy
(``x16.astype(np.float32)``), the oracle's fp32 chain / literal / generator run on them, and the fp32 result
is rounded with ``.astype(np.float16)`` -- round-to-nearest-even, overflow to inf, gradual underflow
(tests/test_f16_cpu.py pins that rule).  Bits are compared (``view(np.uint16)``), except that a NaN only
has to be a NaN: no reference defines its payload.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16, F32 = np.float16, np.float32


def rne16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, F32).astype(F16)


def assert_bits(got, ref, what=""):
    """Same dtype, same bits; NaN positions only have to agree."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    ut = np.uint16 if got.dtype.itemsize == 2 else np.uint32
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), "%s NaN positions differ: %d vs %d" % (what, gn.sum(), rn.sum())
    bad = np.flatnonzero((got.view(ut) != ref.view(ut)) & ~gn)
    assert bad.size == 0, "%s %d/%d mismatches, first at %s: got %s ref %s" % (
        what, bad.size, got.size, bad[:4], got.view(ut)[bad[:4]], ref.view(ut)[bad[:4]])


def tdtype(torch, npdt):
    return torch.float16 if npdt == F16 else torch.float32


def dev_buf(torch, n, npdt, offset=0):
    """n elements starting `offset` elements into a fresh allocation (2-byte aligned only for fp16, offset odd)."""
    return torch.empty(n + 16, dtype=tdtype(torch, npdt), device="cuda")[offset:offset + n]


def to_dev(torch, x, offset=0):
    t = dev_buf(torch, x.size, x.dtype.type, offset)
    t.copy_(torch.from_numpy(x))
    return t


def fa_dt(fa, npdt):
    return fa.F16 if npdt == F16 else fa.F32


def host_f16(O, seed, D, n):
    return [rne16(O.gen(seed, k, n)) for k in range(D)]


def expect(O, xs, w, out, init=None):
    """The ordered fp32 chain over the (exactly widened) inputs, rounded once to `out`."""
    r = O.fedavg([np.ascontiguousarray(x, F32) if x.dtype == F32 else x.astype(F32) for x in xs], w, init=init)
    return rne16(r) if out == F16 else r


def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------ fill

@pytest.mark.parametrize("n", [1, 7, 9, 4099])
def test_fill_f16_matches_the_generator(fa, O, torch_gpu, n):
    torch = torch_gpu
    for client, idx0, off in [(5, 17, 1), (31, (1 << 33) + 3, 0)]:
        t = dev_buf(torch, n + 2, F16, off)
        t.zero_()
        fa.fill_uniform(t[1:], n, fa.F16, 0x5EED, client, idx0)  # 2-byte aligned destination
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        assert_bits(got[1:n + 1], rne16(O.gen(0x5EED, client, n, idx0=idx0)))
        assert got[0] == 0 and got[n + 1] == 0  # nothing outside


# ------------------------------------------------------------------ one-shot and scalar paths

PAIRS = [(F16, F16), (F16, F32), (F32, F16)]
# (offset of client k, output offset): one 16-byte phase shared (vector body with a scalar head and tail),
# the output alone off (f16 -> f16: no vector store), and clients on different phases (one element per lane)
OFFSETS = [(lambda k: 0, 0), (lambda k: 1, 1), (lambda k: 3, 3), (lambda k: 7, 7), (lambda k: 0, 3),
           (lambda k: (0, 1, 3, 7)[k % 4], 1)]


@pytest.mark.parametrize("n", [1, 7, 9, 777, 1_000_003])
def test_reduce_device_f16_pairs(fa, O, torch_gpu, n):
    torch = torch_gpu
    Ds = [1, 2, 8, 9, 17]
    x16 = host_f16(O, 200 + n, max(Ds), n)
    x32 = [O.gen(200 + n, k, n) for k in range(max(Ds))]
    dev = {}  # (dtype, offset, k) -> device bucket, uploaded once

    def client(dt, off, k):
        key = (dt, off, k)
        if key not in dev:
            dev[key] = to_dev(torch, (x16 if dt == F16 else x32)[k], off)
        return dev[key]

    for D in Ds:
        w = O.weights(D)
        ref = {(i, o): expect(O, (x16 if i == F16 else x32)[:D], w, o) for i, o in PAIRS}
        for (i, o) in PAIRS:
            for koff, ooff in OFFSETS:
                out = dev_buf(torch, n, o, ooff)
                fa.reduce_device([client(i, koff(k), k) for k in range(D)], w, n, fa_dt(fa, i), out, fa_dt(fa, o))
                torch.cuda.synchronize()
                assert_bits(out.cpu().numpy(), ref[(i, o)], "D=%d %s->%s out+%d" % (D, i.__name__, o.__name__, ooff))


@pytest.mark.parametrize("n,off", [(777, 0), (777, 1), (1_000_003, 0), (1_000_003, 1)])
def test_init_continues_an_f16_chain(fa, O, torch_gpu, n, off):
    """D = 9 split 4 + 5 with an fp32 hand-off: the bits of one launch."""
    torch = torch_gpu
    D = 9
    w = O.weights(D)
    xs = host_f16(O, 77, D, n)
    clients = [to_dev(torch, x, off) for x in xs]
    one = dev_buf(torch, n, F16, off)
    fa.reduce_device(clients, w, n, fa.F16, one, fa.F16)
    acc = dev_buf(torch, n, F32, off)
    fa.reduce_device(clients[:4], w[:4], n, fa.F16, acc, fa.F32)
    two = dev_buf(torch, n, F16, off)
    fa.reduce_device(clients[4:], w[4:], n, fa.F16, two, fa.F16, init=acc)
    torch.cuda.synchronize()
    ref = expect(O, xs, w, F16)
    assert_bits(one.cpu().numpy(), ref)
    assert_bits(two.cpu().numpy(), ref)
    assert_bits(acc.cpu().numpy(), expect(O, xs[:4], w[:4], F32))


# ------------------------------------------------------------------ specials and rounding

W_SPECIAL = np.array([1.0, 0.5, 2.0 ** -20], F32)  # powers of two: every product is exact in fp32
INF, NAN, MAXH, SUB = np.inf, np.nan, 65504.0, 2.0 ** -24  # SUB: the smallest fp16 subnormal
# (x0, x1, x2) -> the fp32 chain value x0 + x1 / 2 + x2 / 2^20 (exact) and the fp16 bits it rounds to
SPECIAL_CASES = [
    ((0.0, 0.0, 0.0), 0.0, 0x0000),
    ((-0.0, -0.0, -0.0), 0.0, 0x0000),                              # fma(-0, w, +0) = +0
    ((0.0, -SUB, 0.0), -2.0 ** -25, 0x8000),                       # tie below the smallest subnormal -> -0
    ((0.0, 0.0, -2.0 ** -10), -2.0 ** -30, 0x8000),
    ((INF, 1.0, 1.0), INF, 0x7C00),
    ((1.0, -INF, 1.0), -INF, 0xFC00),
    ((INF, -INF, 0.0), NAN, None),
    ((1.0, NAN, 0.0), NAN, None),
    ((SUB * 3, 0.0, 0.0), 2.0 ** -24 * 3, 0x0003),                 # fp16 subnormal inputs, widened exactly
    ((SUB * 1023, SUB * 2, 0.0), 2.0 ** -14, 0x0400),              # subnormals summing to the smallest normal
    ((MAXH, 31.984375, 0.0), 65519.9921875, 0x7BFF),                # 65519.99 -> the largest finite
    ((MAXH, 32.0, 0.0), 65520.0, 0x7C00),                           # the tie at 65520 -> inf
    ((-MAXH, -MAXH, 0.0), -98256.0, 0xFC00),                        # overflow on rounding
    ((SUB, 0.0, 0.0), 2.0 ** -24, 0x0001),
    ((0.0, SUB, 0.0), 2.0 ** -25, 0x0000),                          # the tie at half the smallest subnormal -> even
    ((0.0, SUB, SUB * 2), 2.0 ** -25 * (1 + 2.0 ** -18), 0x0001),  # just above that tie
    ((2.0 ** -14, -SUB, 0.0), 2.0 ** -14 * (1 - 2.0 ** -11), 0x0400),  # tie between the largest subnormal and 2^-14
    ((1.0, 2.0 ** -10, 0.0), 1 + 2.0 ** -11, 0x3C00),               # tie -> even (down)
    ((1.0 + 2.0 ** -10, 2.0 ** -10, 0.0), 1 + 3 * 2.0 ** -11, 0x3C02),  # tie -> even (up)
    ((SUB * 5, SUB * 7, 0.0), 2.0 ** -24 * 8.5, 0x0008),            # a result in the subnormal range, tie -> even
    ((2.0 ** -15, SUB, 1.0), 2.0 ** -15 + 2.0 ** -25 + 2.0 ** -20, 0x0210),  # 528.5 subnormal steps: tie -> even
]


def special_inputs(n):
    rng = np.random.default_rng(16)
    K = len(SPECIAL_CASES)
    xs = [rne16(rng.uniform(-2, 2, n)) for _ in range(3)]
    for k in range(3):  # results in the fp16 subnormal range: x0 + x1 / 2 of subnormal inputs
        m = xs[k][n // 2:: 5].size
        xs[k][n // 2:: 5] = rng.integers(1, 1024, m).astype(np.uint16).view(F16) if k < 2 else 0
    for k in range(3):
        col = np.array([c[0][k] for c in SPECIAL_CASES], F16)
        for s in range(0, n // 2, K):  # tiled: every case meets the scalar head, the vector body and the tail
            m = min(K, n // 2 - s)
            xs[k][s:s + m] = col[:m]
        xs[k][n - K:] = col
    return xs


def test_special_values_and_rounding(fa, O, torch_gpu):
    torch = torch_gpu
    n, K = 4096, len(SPECIAL_CASES)
    xs = special_inputs(n)
    for k in range(3):  # the hand-placed inputs are exact in fp16
        want = np.array([c[0][k] for c in SPECIAL_CASES], np.float64)
        got = xs[k][:K].astype(np.float64)
        assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    r32 = expect(O, xs, W_SPECIAL, F32)
    r16 = rne16(r32)
    # the expectation lands on every named case (chain value and rounded bits), checked before the GPU
    for base in (0, K, n - K):
        for j, (_, chain, bits) in enumerate(SPECIAL_CASES):
            v = r32[base + j]
            if bits is None:
                assert np.isnan(v) and np.isnan(r16[base + j])
            else:
                assert v == F32(chain) and (np.signbit(v) == np.signbit(F32(chain))), (j, v, chain)
                assert r16.view(np.uint16)[base + j] == bits, (j, hex(r16.view(np.uint16)[base + j]), hex(bits))
    sub = (np.abs(r32) < 2.0 ** -14) & (r32 != 0)
    assert sub.sum() > 100 and (r16[sub] != 0).sum() > 50  # results in the fp16 subnormal range, kept
    x32 = [x.astype(F32) for x in xs]
    for (i, o) in PAIRS:
        src = xs if i == F16 else x32
        ref = r16 if o == F16 else r32
        for koff, ooff in OFFSETS:
            clients = [to_dev(torch, src[k], koff(k)) for k in range(3)]
            out = dev_buf(torch, n, o, ooff)
            fa.reduce_device(clients, W_SPECIAL, n, fa_dt(fa, i), out, fa_dt(fa, o))
            torch.cuda.synchronize()
            assert_bits(out.cpu().numpy(), ref, "%s->%s out+%d" % (i.__name__, o.__name__, ooff))
    # literal mode on the same values: fl16(fl32(fl32(x + x) / 1000))
    lit = dev_buf(torch, n, F16)
    fa.reduce_device([to_dev(torch, xs[0])], np.zeros(1, F32), n, fa.F16, lit, fa.F16, fa.LITERAL)
    torch.cuda.synchronize()
    x = xs[0].astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        assert_bits(lit.cpu().numpy(), rne16((x + x) / F32(1000)))


# ------------------------------------------------------------------ D > 128

def test_more_than_128_clients_f16_output_takes_ctx_scratch(fa, O, torch_gpu):
    torch = torch_gpu
    D, n = 130, 50_003
    w = O.weights(D)
    clients = []
    for k in range(D):
        t = dev_buf(torch, n, F16)
        fa.fill_uniform(t, n, fa.F16, 0xF16, k)
        clients.append(t)
    out = dev_buf(torch, n, F16)
    with pytest.raises(fa.FaError) as e:
        fa.reduce_device(clients, w, n, fa.F16, out, fa.F16)
    assert e.value.code == fa.ERR_ARG
    with fa.Aggregator(1) as agg:
        fa.reduce_device(clients, w, n, fa.F16, out, fa.F16, ctx=agg)
        agg.sync()
        torch.cuda.synchronize()
    assert_bits(out.cpu().numpy(), expect(O, host_f16(O, 0xF16, D, n), w, F16))


def test_mixed_16bit_pairs_refused_on_the_device_entries(fa, O, torch_gpu):
    torch = torch_gpu
    a, b = dev_buf(torch, 64, F16), dev_buf(torch, 64, F16)
    for i, o in ((fa.BF16, fa.F16), (fa.F16, fa.BF16)):
        with pytest.raises(fa.FaError) as e:
            fa.reduce_device([a], [1.0], 64, i, b, o)
        assert e.value.code == fa.ERR_ARG and "bf16" in str(e.value) and "f16" in str(e.value).replace("bf16", "")
        with fa.Aggregator(1) as agg:
            with pytest.raises(fa.FaError) as e:
                agg.define(1, 64, i, o, 2)
            assert e.value.code == fa.ERR_ARG and "bf16" in str(e.value)


# ------------------------------------------------------------------ phased kernel

def full_phase_elems(fa, torch, out, D=3):
    """Elements of one full phase of the f16 chain, read from the plan: the smallest bucket of D < 16 clients
    that the planner gives to the phased grid."""
    lo, hi = 1, 1 << 30
    assert fa.plan_chain(fa.F16, out, hi, D, cus=cus(torch))[0] == fa.PLAN_PHASED
    while lo < hi:
        mid = (lo + hi) // 2
        if fa.plan_chain(fa.F16, out, mid, D, cus=cus(torch))[0] == fa.PLAN_PHASED:
            hi = mid
        else:
            lo = mid + 1
    return lo


def sample_idx(n, edges, count=100_000, seed=0):
    rng = np.random.default_rng(seed)
    parts = [np.arange(0, min(n, 4096)), np.arange(max(0, n - 4096), n), rng.integers(0, n, count)]
    for e in edges:  # both sides of every phase boundary
        parts.append(np.arange(max(0, e - 64), min(n, e + 64)))
    return np.unique(np.concatenate(parts)).astype(np.int64)


def sampled_expect(O, seed, w, idx, out):
    xs = [rne16(O.gen_at(seed, k, idx)).astype(F32) for k in range(len(w))]
    r = O.fedavg(xs, w)
    return rne16(r) if out == F16 else r


def filled_f16(fa, torch, n, seed, D):
    cl = []
    for k in range(D):
        t = dev_buf(torch, n, F16)
        fa.fill_uniform(t, n, fa.F16, seed, k)
        cl.append(t)
    return cl


@pytest.mark.parametrize("out", [F16, F32])
@pytest.mark.parametrize("phases", [1.3, 2.2])
def test_phased_f16_chain(fa, O, torch_gpu, out, phases):
    torch = torch_gpu
    D, seed = 3, 1600
    P = full_phase_elems(fa, torch, fa_dt(fa, out))
    n = int(P * phases) + 4_321
    kind, nph = fa.plan_chain(fa.F16, fa_dt(fa, out), n, D, cus=cus(torch))
    assert kind == fa.PLAN_PHASED and nph == int(phases) + 1  # not the one-shot grid
    w = O.weights(D)
    clients = filled_f16(fa, torch, n, seed, D)
    o = dev_buf(torch, n, out)
    fa.reduce_device(clients, w, n, fa.F16, o, fa_dt(fa, out))
    torch.cuda.synchronize()
    idx = sample_idx(n, [P * p for p in range(1, nph)])
    assert idx.size >= 100_000
    got = o[torch.as_tensor(idx, device="cuda")].cpu().numpy()
    assert_bits(got, sampled_expect(O, seed, w, idx, out))
    assert fa.phased_timeouts(0) == 0
    del clients


def test_sized_phase_f16(fa, O, torch_gpu):
    """D = 16 at q = 4 vectors per lane (about 4.2 M elements on 256 CUs): one phase sized to the bucket."""
    torch = torch_gpu
    D, seed = 16, 1700
    n = 4 * cus(torch) * 512 * 8 - 5
    assert fa.plan_chain(fa.F16, fa.F16, n, D, cus=cus(torch)) == (fa.PLAN_PHASED, 1)
    w = O.weights(D)
    clients = filled_f16(fa, torch, n, seed, D)
    o = dev_buf(torch, n, F16)
    fa.reduce_device(clients, w, n, fa.F16, o, fa.F16)
    torch.cuda.synchronize()
    idx = sample_idx(n, [])
    assert idx.size >= 100_000
    assert_bits(o[torch.as_tensor(idx, device="cuda")].cpu().numpy(), sampled_expect(O, seed, w, idx, F16))
    assert fa.phased_timeouts(0) == 0


# ------------------------------------------------------------------ context paths

CTX_N = [50_536, 1_000_003]


@pytest.fixture(scope="module")
def ctx_case(O):
    """Three fp16 receipts per size and their expectation, computed once and left unchanged."""
    cases = {}
    for n in CTX_N:
        xs = host_f16(O, 0xC0 + n % 97, 3, n)
        w = O.weights(3)
        ref = expect(O, xs, w, F16)
        for a in xs + [ref]:
            a.setflags(write=False)
        cases[n] = (xs, w, ref)
    return cases


@pytest.mark.parametrize("n", CTX_N)
def test_ctx_pageable_round(fa, O, torch_gpu, ctx_case, n):
    xs, w, ref = ctx_case[n]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F16, fa.F16, 3)
        for k in (2, 0, 1):
            agg.submit(1, k, xs[k], w[k])
        got = agg.finalize(1)
        assert got.dtype == F16  # the binding's view of an fp16 output
        assert_bits(got, ref)
        assert_bits(agg.copy_output(1), ref)


@pytest.mark.parametrize("n", CTX_N)
def test_ctx_pinned_round(fa, O, torch_gpu, ctx_case, n):
    xs, w, ref = ctx_case[n]
    frames = [fa.PinnedBuffer(2 * n + 16) for _ in xs]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F16, fa.F16, 3)
        for k in range(3):
            v = frames[k].view(F16, count=n, offset=2)  # element-aligned, not 16-byte aligned
            v[:] = xs[k]
            agg.submit(1, k, v, w[k], pinned=True)
        small = 3 * n * 2 <= (1 << 20)  # FA_HOST_READ_MAX_BYTES: the round is read where it lies
        assert agg.host_read_kept(1) == small
        before = agg.host_reads()
        assert_bits(agg.finalize(1), ref)
        assert agg.host_reads() == before + (1 if small else 0)
    for f in frames:
        f.close()


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("n", CTX_N)
def test_ctx_gather_in_and_out(fa, O, torch_gpu, ctx_case, n, pinned):
    xs, w, ref = ctx_case[n]
    cuts = [0, 5, 4096, n // 3, n // 3 + 1, n]
    size = 13 + 2 * n + 70 * len(cuts)
    frames = [fa.PinnedBuffer(size) if pinned else None for _ in xs]
    pieces = []
    for k, x in enumerate(xs):
        raw = frames[k].view() if pinned else np.empty(size, np.uint8)
        ps, off = [], 14  # records at 2-byte aligned places of a frame, as an archive's are at 64
        for a, b in zip(cuts, cuts[1:]):
            seg = raw[off:off + 2 * (b - a)]
            seg[:] = x[a:b].view(np.uint8)
            ps.append(seg)
            off += 2 * (b - a) + 64 - (2 * (b - a)) % 64 + 2
        pieces.append(ps)
    reply = fa.PinnedBuffer(2 * n + 100) if pinned else None
    rraw = reply.view() if pinned else np.zeros(2 * n + 100, np.uint8)
    rraw[:] = 0
    ocuts = [0, 1, n // 2, n]
    outs = [rraw[8 + 2 * a: 8 + 2 * b] for a, b in zip(ocuts, ocuts[1:])]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F16, fa.F16, 3)
        for k in range(3):
            agg.submit_gather(1, k, pieces[k], w[k], pinned=pinned)
        agg.finalize_gather(1, outs, pinned=pinned)
        assert_bits(np.concatenate([o.view(F16) for o in outs]), ref)
        assert not rraw[:8].any() and not rraw[8 + 2 * n:].any()
    for f in frames + [reply]:
        if f:
            f.close()


@pytest.mark.parametrize("n", CTX_N)
def test_ctx_pieces_and_commit(fa, O, torch_gpu, ctx_case, n):
    xs, w, ref = ctx_case[n]
    cuts = [0, 2400, 2416, n // 2, n]
    frames = [fa.PinnedBuffer(2 * n + 64) for _ in xs]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F16, fa.F16, 3)
        for k, x in enumerate(xs):
            v = frames[k].view(F16, count=n, offset=32)
            v[:] = x
            for a, b in reversed(list(zip(cuts, cuts[1:]))):  # any order, as records arrive
                agg.submit_piece(1, k, 2 * a, v[a:b])
            agg.submit_commit(1, k, w[k])
        assert_bits(agg.finalize(1), ref)
    for f in frames:
        f.close()


@pytest.mark.parametrize("max_d", [8, 16])
def test_reduce_parts_three_f16_parts_one_launch(fa, O, torch_gpu, max_d):
    parts = {2: (50_536, max_d), 3: (7, 3), 4: (10_164, 5)}
    with fa.Aggregator(1) as agg:
        refs = {}
        for pid, (n, D) in parts.items():
            agg.define(pid, n, fa.F16, fa.F16, D)
            xs, w = host_f16(O, 300 + pid, D, n), O.weights(D)
            for k in range(D):
                agg.submit(pid, k, xs[k], w[k])
            refs[pid] = expect(O, xs, w, F16)
        agg.reduce_parts(list(parts))
        for pid in parts:
            assert_bits(agg.finalize(pid), refs[pid], "part %d" % pid)


def test_accumulate_on_arrival_f16(fa, O, torch_gpu):
    n, D = 1_000_003, 5
    xs, w = host_f16(O, 91, D, n), O.weights(D)
    with fa.Aggregator(1, eager=True) as agg:
        agg.define(1, n, fa.F16, fa.F16, D)
        for k in (3, 0, 4, 1, 2):
            agg.submit(1, k, xs[k], w[k])
        assert_bits(agg.finalize(1), expect(O, xs, w, F16))


@pytest.mark.parametrize("in_dt", [F16, F32])
def test_rs_layout_one_gpu_f16_output(fa, O, torch_gpu, in_dt):
    """FA_SHARD_CLIENT_RS at one GPU is bit-exact: the fp32 shard rounded once to fp16 after the exchange."""
    n, D = 300_001, 4
    xs = host_f16(O, 92, D, n) if in_dt == F16 else [O.gen(92, k, n) for k in range(D)]
    w = O.weights(D)
    with fa.Aggregator(1, rs=True) as agg:
        agg.set_tuning(rs_chunks=3)
        agg.define(1, n, fa_dt(fa, in_dt), fa.F16, D)
        for k in range(D):
            agg.submit(1, k, xs[k], w[k])
        assert_bits(agg.finalize(1), expect(O, xs, w, F16))


def test_range_layout_two_shards_f16(fa, O, torch_gpu, ctx_case):
    n = CTX_N[1]
    xs, w, ref = ctx_case[n]
    ctx = fa.Aggregator(2) if fa.device_count() >= 2 else fa.Aggregator(devices=[0, 0], shared_device=True)
    with ctx as agg:
        agg.define(1, n, fa.F16, fa.F16, 3)
        for k in range(3):
            agg.submit(1, k, xs[k], w[k])
        assert_bits(agg.finalize(1), ref)


def test_output_crc32_of_an_f16_output(fa, O, torch_gpu, ctx_case):
    n = CTX_N[1]
    xs, w, ref = ctx_case[n]
    rng = np.random.default_rng(5)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F16, fa.F16, 3)
        for k in range(3):
            agg.submit(1, k, xs[k], w[k])
        agg.reduce(1)
        agg.sync()
        raw = agg.copy_output(1).tobytes()
        assert raw == ref.tobytes()
        for k in (1, 2, 17, 300):
            cut = np.sort(rng.integers(0, len(raw) + 1, k - 1)) if k > 1 else np.array([], np.int64)
            edges = np.concatenate([[0], cut, [len(raw)]]).astype(np.int64)
            seg = [int(b - a) for a, b in zip(edges[:-1], edges[1:])]
            o = 0
            for c, L in zip(agg.output_crc32(1, seg), seg):
                assert c == zlib.crc32(raw[o:o + L]) & 0xFFFFFFFF, (o, L)
                o += L


@pytest.mark.parametrize("n", CTX_N)
def test_literal_mode_f16(fa, O, torch_gpu, ctx_case, n):
    xs, _, _ = ctx_case[n]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F16, fa.F16, 3, fa.LITERAL)
        for k in (2, 0, 1):
            agg.submit(1, k, xs[k])
        x = xs[1].astype(F32)
        assert_bits(agg.finalize(1), ((x + x) / F32(1000)).astype(F16))


# ------------------------------------------------------------------ state sync

@pytest.mark.parametrize("D", [2, 9, 130])
def test_sync_device_f16(fa, O, torch_gpu, D):
    torch = torch_gpu
    n = 100_003
    w = O.weights(D)
    xs = host_f16(O, 62, D, n)
    slots = filled_f16(fa, torch, n, 62, D)
    with fa.Aggregator(1) as agg:
        fa.sync_device(slots, w, n, fa.F16, ctx=agg if D > 128 else None)
        agg.sync()
        torch.cuda.synchronize()
    ref = expect(O, xs, w, F16)
    for k in range(D):
        assert_bits(slots[k].cpu().numpy(), ref, "slot %d" % k)


def test_sync_device_f16_phased(fa, O, torch_gpu):
    torch = torch_gpu
    D, seed = 3, 63
    P = full_phase_elems(fa, torch, fa.F16)  # the sync's phase is the f16 -> f16 chain's
    n = int(P * 1.3) + 4_321
    w = O.weights(D)
    slots = filled_f16(fa, torch, n, seed, D)
    fa.sync_device(slots, w, n, fa.F16)
    torch.cuda.synchronize()
    for k in range(1, D):
        assert torch.equal(slots[0].view(torch.int16), slots[k].view(torch.int16)), "slot %d differs" % k
    idx = sample_idx(n, [P])
    assert_bits(slots[0][torch.as_tensor(idx, device="cuda")].cpu().numpy(), sampled_expect(O, seed, w, idx, F16))
    assert fa.phased_timeouts(0) == 0
