"""GPU: FA_TRIMMED (coordinate-wise trimmed mean / median) bit for bit against tests/trimmed_ref.py.

Every comparison covers all elements; where the expected value is NaN only a NaN is required.
"""
import zlib

import numpy as np
import pytest

import trimmed_ref as T

pytestmark = pytest.mark.gpu

F16, F32, U16 = np.float16, np.float32, np.uint16
SEED = 0x7121
NS = [1, 7, 67, 4099, 100003]


def host_inputs(O, D, n, kind="f32", seed=SEED):
    xs = [O.gen(seed, k, n) for k in range(D)]
    if kind == "f16":
        return [x.astype(F16) for x in xs]
    if kind == "bf16":
        return [T.f32_to_bf16(x) for x in xs]
    return xs


def to_dev(torch, x, offset=0):
    """x on the device, `offset` elements into a fresh allocation."""
    if x.dtype == U16:
        t = torch.empty(x.size + 16, dtype=torch.bfloat16, device="cuda")[offset:offset + x.size]
        t.copy_(torch.from_numpy(x.view(np.int16)).view(torch.bfloat16))
    else:
        t = torch.empty(x.size + 16, dtype=torch.float16 if x.dtype == F16 else torch.float32,
                        device="cuda")[offset:offset + x.size]
        t.copy_(torch.from_numpy(x))
    return t


def dev_out(torch, n, kind, offset=0):
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind]
    return torch.zeros(n + 16, dtype=dt, device="cuda")[offset:offset + n]


def to_host(torch, t, kind):
    if kind == "bf16":
        return t.view(torch.int16).cpu().numpy().view(U16)
    return t.cpu().numpy()


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def trims_for(D):
    return sorted({t for t in (0, 1, (D - 1) // 2) if 2 * t < D})


def run_raw(fa, torch, devs, n, ikind, okind, trim, out_offset=0):
    out = dev_out(torch, n, okind, out_offset)
    fa.trimmed_device([d[:n] for d in devs], n, fa_dt(fa, ikind), out, fa_dt(fa, okind), trim=trim)
    torch.cuda.synchronize()
    return to_host(torch, out, okind)


# ------------------------------------------------------------------ raw entry

@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 128])
def test_raw_entry_parity(fa, O, torch_gpu, D):
    torch = torch_gpu
    xs = host_inputs(O, D, max(NS))
    devs = [to_dev(torch, x) for x in xs]
    for n in NS:
        for t in trims_for(D):
            ref = T.trimmed([x[:n] for x in xs], t)
            for trim in ([t, fa.TRIM_MEDIAN] if t == (D - 1) // 2 else [t]):
                got = run_raw(fa, torch, devs, n, "f32", "f32", trim)
                T.assert_bits(got, ref, "D %d n %d trim %d" % (D, n, trim))


PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("f16", "f32"),
         ("f32", "f16")]


@pytest.mark.parametrize("D", [5, 32])
def test_raw_entry_dtype_pairs(fa, O, torch_gpu, D):
    torch = torch_gpu
    n = 4099
    for ikind in ("f32", "bf16", "f16"):
        xs = host_inputs(O, D, n, ikind)
        devs = [to_dev(torch, x) for x in xs]
        for okind in [o for i, o in PAIRS if i == ikind]:
            for t in trims_for(D):
                ref = T.trimmed(xs, t, in_bf16=ikind == "bf16", out=okind)
                T.assert_bits(run_raw(fa, torch, devs, n, ikind, okind, t), ref, "%s->%s D %d trim %d" % (ikind, okind, D, t))


@pytest.mark.parametrize("ikind", ["f32", "f16"])
def test_raw_entry_unaligned_and_mixed_phases(fa, O, torch_gpu, ikind):
    torch = torch_gpu
    D, n = 9, 4099
    xs = host_inputs(O, D, n, ikind)
    ref = T.trimmed(xs, 1, out=ikind)
    one_off = [to_dev(torch, x, 1) for x in xs]  # one shared phase: vector body with a scalar head and tail
    T.assert_bits(run_raw(fa, torch, one_off, n, ikind, ikind, 1, out_offset=1), ref, "offset 1")
    mixed = [to_dev(torch, x, (0, 1, 3, 2)[k % 4]) for k, x in enumerate(xs)]  # one element per lane
    T.assert_bits(run_raw(fa, torch, mixed, n, ikind, ikind, 1), ref, "mixed phases")
    T.assert_bits(run_raw(fa, torch, one_off, n, ikind, ikind, 1, out_offset=3), ref, "output phase alone off")


def special_columns(n, D=8):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (D, n)).astype(F32)
    c = np.arange(n) % 16
    x[0, c == 1] = np.nan
    x[0, c == 2] = np.nan
    x[5, c == 2] = -np.nan
    x[1, c == 3] = np.inf
    x[2, c == 3] = -np.inf
    x[:, c == 4] = np.where(np.arange(D)[:, None] % 2, F32(-0.0), F32(0.0))
    x[:, c == 5] = F32(0.375)
    x[:, c == 6] = (rng.integers(-64, 64, (D, (c == 6).sum())).astype(F32) * F32(1.4e-45))  # subnormals
    x[:4, c == 7] = F32(3e38)
    x[4:, c == 7] = F32(-3e38)
    x[:, c == 8] = F32(-0.0)
    x[3, c == 9] = np.inf
    x[6, c == 9] = np.inf
    return [np.ascontiguousarray(r) for r in x]


@pytest.mark.parametrize("okind", ["f32", "f16"])
def test_raw_entry_specials(fa, torch_gpu, okind):
    torch = torch_gpu
    n = 4099
    xs = special_columns(n)
    if okind == "f16":  # values that round past 65504
        for k, x in enumerate(xs):
            x[np.arange(n) % 16 == 10] = F32(65504.0 + 8.0 * k)
            x[np.arange(n) % 16 == 11] = F32(65520.0)
    devs = [to_dev(torch, x) for x in xs]
    for t in (0, 1, 3):
        ref = T.trimmed(xs, t, out=okind)
        T.assert_bits(run_raw(fa, torch, devs, n, "f32", okind, t), ref, "specials trim %d" % t)


def test_survives_a_garbage_owner_where_fedavg_does_not(fa, O, torch_gpu):
    torch = torch_gpu
    D, n = 8, 4099
    xs = host_inputs(O, D, n)
    xs[2] = np.full(n, np.nan, F32)
    xs[6] = np.full(n, 1e30, F32)
    devs = [to_dev(torch, x) for x in xs]
    got = run_raw(fa, torch, devs, n, "f32", "f32", 1)
    assert np.all(np.isfinite(got))
    T.assert_bits(got, T.trimmed(xs, 1), "robust")
    out = dev_out(torch, n, "f32")
    fa.reduce_device(devs, O.weights(D), n, fa.F32, out, fa.F32, fa.FEDAVG)
    torch.cuda.synchronize()
    assert np.all(np.isnan(out.cpu().numpy()))


# ------------------------------------------------------------------ through Aggregator

def test_aggregator_round_gather_crc_and_set_trim(fa, O, torch_gpu):
    D, n = 5, 4099
    xs = host_inputs(O, D, n)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        pins = [fa.PinnedBuffer(n * 4) for _ in range(D)]
        for k in range(D):
            if k % 2:
                pins[k].view(F32)[:] = xs[k]
                agg.submit(1, k, pins[k].view(F32), pinned=True)  # small enough that FedAvg would keep it host-side
            else:
                agg.submit(1, k, xs[k])
        assert agg.host_read_kept(1) == 0
        ref_med = T.trimmed(xs)
        T.assert_bits(agg.finalize(1), ref_med, "median round")
        # the device output: CRC-32 of three byte segments equals zlib's over the result
        seg = [4 * 1000, 4 * 99, 4 * 3000]
        assert agg.output_crc32(1, seg) == [zlib.crc32(ref_med.tobytes()[sum(seg[:i]):sum(seg[:i + 1])]) for i in range(3)]
        # next round: trim 1, gathered into three pinned segments
        agg.set_trim(1, 1)
        for k in range(D):
            agg.submit(1, k, xs[k])
        outp = fa.PinnedBuffer(n * 4)
        v = outp.view(F32)
        agg.finalize_gather(1, [v[:1000], v[1000:1099], v[1099:]], pinned=True)
        ref1 = T.trimmed(xs, 1)
        T.assert_bits(v.copy(), ref1, "trim 1 round")
        assert not np.array_equal(ref1.view(np.uint32), ref_med.view(np.uint32))


def test_aggregator_two_range_shards_and_pieces(fa, O, torch_gpu):
    D, n = 5, 100003
    xs = host_inputs(O, D, n)
    ref = T.trimmed(xs, 1)
    with fa.Aggregator(devices=[0, 0], shared_device=True) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED, trim=1)
        for k in range(D):
            agg.submit(1, k, xs[k])
        T.assert_bits(agg.finalize(1), ref, "two range shards")
    with fa.Aggregator(1) as agg:
        agg.set_tuning(piece_span_kib=512, piece_split_kib=-1)  # 5 slots x 128 K elements per piece
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED, trim=1)
        assert len(agg.pieces(1, 0, 0)) >= 3
        for k in range(D):
            agg.submit(1, k, xs[k])
        T.assert_bits(agg.finalize(1), ref, "range pieces")


def test_reduce_parts_mixed_and_eager(fa, O, torch_gpu):
    D, n = 4, 4099
    xs = host_inputs(O, D, n)
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED, trim=1)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.define(3, 67, fa.F32, fa.F32, D)
        for k in range(D):
            agg.submit(1, k, xs[k], w[k])
            agg.submit(2, k, xs[k], w[k])
            agg.submit(3, k, xs[k][:67], w[k])
        agg.reduce_parts([1, 2, 3])
        T.assert_bits(agg.finalize(1), T.trimmed(xs, 1), "trimmed part")
        assert np.array_equal(agg.finalize(2).view(np.uint32), O.fedavg(xs, w).view(np.uint32))
        assert np.array_equal(agg.finalize(3).view(np.uint32), O.fedavg([x[:67] for x in xs], w).view(np.uint32))
    with fa.Aggregator(1, eager=True) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        for k in range(D):
            agg.submit(1, k, xs[k])
        assert agg.progress(1) == (D, 0)  # nothing reduced before the finalize
        T.assert_bits(agg.finalize(1), T.trimmed(xs), "eager context")


def test_refusals_leave_the_context_usable(fa, O, torch_gpu):
    D, n = 4, 67
    xs = host_inputs(O, D, n)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        assert e.value.code == fa.ERR_ARG
        agg.define(1, n, fa.F32, fa.F32, D)  # still usable
    with fa.Aggregator(1) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.define(1, n, fa.F32, fa.F32, 129, mode=fa.TRIMMED)
        assert e.value.code == fa.ERR_ARG
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        with pytest.raises(fa.FaError) as e:
            agg.set_trim(2, 1)
        assert e.value.code == fa.ERR_ARG and "4" in str(e.value)
        for k in range(D):
            agg.submit(1, k, xs[k])
        T.assert_bits(agg.finalize(1), T.trimmed(xs), "after refusals")
