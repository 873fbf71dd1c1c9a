"""GPU: the noise stage (fa.h "Noise stage") against tests/noise_ref.py, every bit.

The raw entry over sizes, output forms, pointer phases of both operands and bucket offsets (together every
(pointer phase, group phase) pair of the vector form and of the element form, and a size at which a wave walks
more than one tile per chunk); IEEE edge inputs; the same bits from range shards and range pieces; the stage
between the clip / Krum / trimmed aggregate and the server optimizer over three rounds; the refusals.
"""
import numpy as np
import pytest

import clip_ref as R
import krum_ref as K
import noise_ref as N
import server_opt_ref as S
import trimmed_ref as T

pytestmark = pytest.mark.gpu

F16, F32, U16, U32 = np.float16, np.float32, np.uint16, np.uint32
SEED = 0x5EEDFACE12345678
NS = [1, 7, 67, 4099, 100003]
IDX0S = [0, 1, 2, 3, 2 ** 34 - 6]
PAD = 8  # sentinel elements either side of a device operand
NMAX = max(NS)


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def np_dt(kind):
    return {"f32": F32, "f16": F16, "bf16": U16}[kind]


def t_dt(torch, kind):
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.int16}[kind]


@pytest.fixture(scope="module")
def aggregate():
    """NMAX fp32 "aggregates" in [-1, 1): shared, never written."""
    a = np.random.default_rng(0xA66).uniform(-1, 1, NMAX).astype(F32)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def normals():
    """idx0 -> the NMAX unit normals of elements idx0 ..; a shorter run is a prefix."""
    cache = {}

    def get(idx0, stream=3, rnd=5):
        key = (idx0, stream, rnd)
        if key not in cache:
            cache[key] = N.normals(SEED, stream, rnd, idx0, NMAX)
            cache[key].setflags(write=False)
        return cache[key]
    return get


def padded(torch, host, kind, offset, fill):
    """A device buffer of PAD + offset sentinels, `host`, PAD sentinels; returns (whole, the view of host)."""
    whole = torch.full((PAD + offset + host.size + PAD,), fill, dtype=t_dt(torch, kind), device="cuda")
    view = whole[PAD + offset:PAD + offset + host.size]
    src = host.view(np.int16) if kind == "bf16" else host
    view.copy_(torch.from_numpy(np.array(src)))  # a copy: the shared inputs are read-only
    return whole, view


def host_of(t, kind):
    h = t.cpu().numpy()
    return h.view(U16) if kind == "bf16" else h


def run_raw(fa, torch, a, okind, alias, avg_off, out_off, stddev, stream, rnd, idx0, ctx=None):
    """One fa_noise_device launch; returns (the output, whether every sentinel survived, the input afterwards)."""
    n = a.size
    wa, va = padded(torch, a, "f32", avg_off, 77.0)
    if alias:
        wo, vo = wa, va
    else:
        wo, vo = padded(torch, np.zeros(n, np_dt(okind)), okind, out_off, 0x55 if okind == "bf16" else 77.0)
    before = host_of(wo, okind).copy()
    fa.noise_device(va, n, vo, fa_dt(fa, okind), stddev, SEED, stream, rnd, idx0, ctx=ctx)
    torch.cuda.synchronize()
    after = host_of(wo, okind)
    lo = PAD + (avg_off if alias else out_off)
    intact = np.array_equal(after[:lo].view(np.uint8), before[:lo].view(np.uint8)) and np.array_equal(
        after[lo + n:].view(np.uint8), before[lo + n:].view(np.uint8))
    return after[lo:lo + n].copy(), intact, host_of(va, "f32")


# ------------------------------------------------------------------ raw entry

@pytest.mark.parametrize("form", ["f32", "f32 aliased", "bf16", "f16"])
@pytest.mark.parametrize("idx0", IDX0S)
def test_raw_entry_sizes_phases_and_offsets(fa, torch_gpu, aggregate, normals, idx0, form):
    okind, alias = form.split()[0], form.endswith("aliased")
    stddev = 0.37
    z = normals(idx0)
    for n in NS:
        a = aggregate[:n]
        want = R.round_out(N.apply(a, stddev, z[:n]), okind)
        for avg_off in range(4):
            for out_off in ([avg_off] if alias else range(4)):
                got, intact, a_after = run_raw(fa, torch_gpu, a, okind, alias, avg_off, out_off, stddev, 3, 5, idx0)
                what = "%s n %d avg+%d out+%d idx0 %d" % (form, n, avg_off, out_off, idx0)
                R.assert_bits(got, want, what)
                assert intact, what + ": wrote outside the output"
                if not alias:
                    R.assert_bits(a_after, a, what + ": the input changed")


@pytest.mark.parametrize("tuning", [dict(), dict(max_blocks=3), dict(block=64), dict(block=128, max_blocks=5)])
@pytest.mark.parametrize("idx0", [0, 1, 2 ** 34 - 6])
def test_raw_entry_many_tiles_per_chunk(fa, torch_gpu, idx0, tuning):
    """A size at which a wave's chunk holds two tiles, the last chunk one: lane 63 takes its upper neighbour's
    normals from the next tile's lane 0, and the grid strides over the chunks when it is capped."""
    n = 2_200_259
    a = np.random.default_rng(n).uniform(-1, 1, n).astype(F32)
    want = N.apply(a, 0.5, N.normals(SEED, 9, 1, idx0, n))
    t = torch_gpu.from_numpy(a).cuda()
    with fa.Aggregator(1) as agg:
        if tuning:
            agg.set_tuning(**tuning)
        fa.noise_device(t, n, t, fa.F32, 0.5, SEED, 9, 1, idx0, ctx=agg)
        torch_gpu.cuda.synchronize()
    R.assert_bits(t.cpu().numpy(), want, "n %d idx0 %d %s" % (n, idx0, tuning))


def test_raw_entry_is_cut_anywhere(fa, torch_gpu, aggregate, normals):
    """Two launches over [0, cut) and [cut, n) give the bits of one."""
    n, idx0 = 4099, 2
    a = aggregate[:n]
    want = N.apply(a, 0.37, normals(idx0)[:n])
    for cut in (1, 2, 3, 5, 1022, 4098):
        t = torch_gpu.from_numpy(a.copy()).cuda()
        fa.noise_device(t[:cut], cut, t[:cut], fa.F32, 0.37, SEED, 3, 5, idx0)
        fa.noise_device(t[cut:], n - cut, t[cut:], fa.F32, 0.37, SEED, 3, 5, idx0 + cut)
        torch_gpu.cuda.synchronize()
        R.assert_bits(t.cpu().numpy(), want, "cut at %d" % cut)


# ------------------------------------------------------------------ edge inputs

def specials(n):
    pats = np.asarray([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F800000,
                       0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000, 0x33800000, 0x477FE000], U32)
    return np.resize(pats, n).view(F32)


@pytest.mark.parametrize("okind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("stddev", [1.0, 1e-40, 3e-39, 2e4, 1e38])
def test_edge_inputs(fa, torch_gpu, normals, okind, stddev):
    """+-0, subnormals, +-inf, NaN and the largest finite values under a unit stddev, one whose products are all
    subnormal, one whose products straddle the smallest normal, one that takes an f16 output beyond 65504 and one
    that overflows fp32 itself."""
    n = 4099
    a = specials(n)
    z = normals(1)[:n]
    with np.errstate(all="ignore"):
        f32_want = N.apply(a, stddev, z)
    if stddev == 1e-40:
        prod = (F32(stddev) * z).view(U32) & U32(0x7F800000)
        assert not prod.any()  # every stddev * z is subnormal or zero
    if stddev == 2e4 and okind == "f16":
        assert np.isinf(R.round_out(f32_want, "f16")[np.isfinite(f32_want)]).any()
    want = R.round_out(f32_want, okind)
    for off in (0, 1):
        got, intact, _ = run_raw(fa, torch_gpu, a, okind, False, off, off, stddev, 3, 5, 1)
        R.assert_bits(got, want, "%s stddev %g +%d" % (okind, stddev, off))
        assert intact


# ------------------------------------------------------------------ through a context: layouts

def make_clients(n, D, kind, seed):
    rng = np.random.default_rng(seed)
    return [R.round_out(rng.uniform(-1, 1, n).astype(F32), kind) for _ in range(D)]


def submit_all(agg, part, xs, w):
    for k, x in enumerate(xs):
        agg.submit(part, k, x, w[k])


def plain_aggregate(O, xs, kind, w):
    if kind == "bf16":
        return O.fedavg([np.ascontiguousarray(x) for x in xs], w, out_dtype="f32")
    return O.fedavg([R.widen(x, kind) for x in xs], w)


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_layout_independence(fa, O, torch_gpu, kind):
    """One GPU, three range shards and forced range pieces give the same bits: those of the reference."""
    D, n, stddev, part = 3, 100003, 0.25, 4
    w = O.weights(D)
    xs = make_clients(n, D, kind, 11)
    want = R.round_out(N.noisy(plain_aggregate(O, xs, kind, w), stddev, SEED, part, 0), kind)
    outs = {}
    for name, mk in (("one GPU", lambda: fa.Aggregator(1)),
                     ("three shards", lambda: fa.Aggregator(devices=[0, 0, 0], shared_device=True)),
                     ("pieces", lambda: fa.Aggregator(1))):
        with mk() as agg:
            if name == "pieces":
                agg.set_tuning(piece_span_kib=64, piece_split_kib=-1)
            agg.set_noise(stddev, SEED)  # the context default
            agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
            if name == "pieces":
                assert len(agg.pieces(part, 0, 0)) >= 3
            assert agg.noise(part) == (np.float32(stddev), SEED) and agg.noise_round(part) == 0
            submit_all(agg, part, xs, w)
            outs[name] = agg.finalize(part)
            assert agg.noise_round(part) == 1
        R.assert_bits(outs[name], want, "%s %s" % (kind, name))


# ------------------------------------------------------------------ composition over three rounds

def test_clip_noise_adam_bf16(fa, O, torch_gpu):
    D, n, C, stddev, part = 3, 4099, float(F32(0.05 * np.sqrt(4099))), 0.01, 2
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    w = O.weights(D)
    rng = np.random.default_rng(21)
    with fa.Aggregator(1) as agg:
        agg.define(part, n, fa.BF16, fa.BF16, D)
        agg.set_noise(stddev, SEED, part)  # any call order: noise, clip, optimizer
        agg.set_clip(C, part)
        agg.set_server_opt(S.ADAM, part_id=part, **hp)
        x0 = rng.uniform(-1, 1, n).astype(F32)
        agg.set_server_opt_state(part, x=x0)
        g = R.widen(R.round_out(x0, "bf16"), "bf16")
        agg.set_clip_reference(part, g)
        ref = (x0, np.zeros(n, F32), np.zeros(n, F32))
        for rnd in range(3):
            assert agg.noise_round(part) == rnd
            xs = [R.round_out((g + F32(0.5 if k % 2 else 0.01) * rng.uniform(0.5, 1.0, n).astype(F32)).astype(F32), "bf16")
                  for k in range(D)]
            submit_all(agg, part, xs, w)
            assert agg.host_read_kept(part) == 0
            if rnd == 1:
                agg.reduce(part)
                out = agg.copy_output(part)
            else:
                out = agg.finalize(part)
            Q, scales, included, n_clipped = agg.clip_round(part)
            assert 0 < n_clipped < D
            a = N.noisy(R.aggregate(O, xs, "bf16", w, scales, included, g), stddev, SEED, part, rnd)
            ref = S.step(S.ADAM, a, *ref, **hp)
            x, m, v, steps = agg.server_opt_state(part)
            assert steps == rnd + 1
            for got, exp, name in ((x, ref[0], "x"), (m, ref[1], "m"), (v, ref[2], "v")):
                R.assert_bits(got, exp, "round %d %s" % (rnd, name))
            R.assert_bits(out, S.round_out(ref[0], "bf16"), "round %d output" % rnd)
            g = R.widen(out, "bf16")
            R.assert_bits(agg.clip_reference(part), g, "round %d reference: what the owners receive" % rnd)
        assert agg.noise_round(part) == 3


@pytest.mark.parametrize("kind,okind", [("f32", "f32"), ("f32", "bf16"), ("f16", "f16")])
def test_clip_bootstrap_round_is_noisy_and_becomes_the_reference(fa, O, torch_gpu, kind, okind):
    D, n, stddev, part = 3, 4099, 0.125, 1
    w = O.weights(D)
    xs = make_clients(n, D, kind, 31)
    with fa.Aggregator(1) as agg:
        agg.set_clip(1.0)
        agg.set_noise(stddev, SEED)
        agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, okind), D)
        submit_all(agg, part, xs, w)
        out = agg.finalize(part)
        R.assert_bits(out, R.round_out(N.noisy(plain_aggregate(O, xs, kind, w), stddev, SEED, part, 0), okind), "bootstrap")
        R.assert_bits(agg.clip_reference(part), R.widen(out, okind), "reference: noise included")


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_krum_noise(fa, O, torch_gpu, kind):
    D, f, n, stddev = 5, 1, 4099, 0.05
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        for part in (1, 2):
            agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
            agg.set_krum(f, None, part)
            agg.set_noise(stddev, SEED, part)
        outs = {}
        for rnd in range(3):
            xs = make_clients(n, D, kind, 41 + rnd)
            xs[rnd] = R.round_out((R.widen(xs[rnd], kind) + F32(30.0)).astype(F32), kind)  # one owner far away
            for part in (1, 2):
                assert agg.noise_round(part) == rnd
                submit_all(agg, part, xs, w)
                outs[part] = agg.finalize(part)
                _, _, sel = agg.krum_round(part)
                assert not sel[rnd] and sel.sum() == D - f
                a = K.aggregate(O, xs, kind, w, sel)
                R.assert_bits(outs[part], R.round_out(N.noisy(a, stddev, SEED, part, rnd), kind), "part %d round %d" % (part, rnd))
            # one seed, two parts: the part id is the stream
            assert (outs[1].view(np_dt(kind)) != outs[2].view(np_dt(kind))).mean() > 0.9
        # replay round 1 of part 1 bit for bit
        xs = make_clients(n, D, kind, 41 + 1)
        xs[1] = R.round_out((R.widen(xs[1], kind) + F32(30.0)).astype(F32), kind)
        agg.set_noise_round(1, 1)
        submit_all(agg, 1, xs, w)
        replay = agg.finalize(1)
        _, _, sel = agg.krum_round(1)
        R.assert_bits(replay, R.round_out(N.noisy(K.aggregate(O, xs, kind, w, sel), stddev, SEED, 1, 1), kind), "replay")
        assert agg.noise_round(1) == 2


@pytest.mark.parametrize("kind,okind", [("f32", "f32"), ("f16", "f16"), ("bf16", "f32")])
def test_trimmed_noise_then_removed(fa, O, torch_gpu, kind, okind):
    D, n, stddev, part = 5, 4099, 0.05, 6
    with fa.Aggregator(1) as agg:
        agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, okind), D, mode=fa.TRIMMED, trim=1)
        agg.set_noise(stddev, SEED, part)
        w = O.weights(D)
        for rnd in range(3):
            xs = make_clients(n, D, kind, 51 + rnd)
            submit_all(agg, part, xs, w)
            if rnd == 2:
                agg.reduce_parts([part])
            out = agg.finalize(part)
            a = T.trimmed_f32([R.widen(x, kind) for x in xs], 1)
            R.assert_bits(out, R.round_out(N.noisy(a, stddev, SEED, part, rnd), okind), "round %d" % rnd)
        agg.set_noise(2 * stddev, SEED + 1, part)  # again: new stddev and seed, the round stays
        assert agg.noise(part) == (np.float32(2 * stddev), SEED + 1) and agg.noise_round(part) == 3
        submit_all(agg, part, xs, w)
        R.assert_bits(agg.finalize(part), R.round_out(N.noisy(a, 2 * stddev, SEED + 1, part, 3), okind), "new seed")
        agg.set_noise(0.0, 0, part)  # removed: the bits of a part that never had the stage
        assert agg.noise(part)[0] == 0.0
        with pytest.raises(fa.FaError) as e:
            agg.noise_round(part)
        assert e.value.code == fa.ERR_STATE
        submit_all(agg, part, xs, w)
        R.assert_bits(agg.finalize(part), R.round_out(a, okind), "stage removed")


def test_reduce_parts_with_a_noise_part_among_plain_ones(fa, O, torch_gpu):
    D, n, stddev = 3, 4099, 0.5
    w = O.weights(D)
    xs = make_clients(n, D, "f32", 61)
    with fa.Aggregator(1, eager=True) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.define(3, n, fa.F32, fa.BF16, D)
        agg.set_noise(stddev, SEED, 2)
        agg.set_noise(stddev, SEED, 3)
        agg.submit(2, 0, xs[0], w[0])
        with pytest.raises(fa.FaError) as e:  # a noise part needs every client
            agg.reduce_parts([1, 2], weights=[w, w])
        assert e.value.code == fa.ERR_STATE
        pins = [fa.PinnedBuffer(n * 4) for _ in range(D)]
        for k in range(D):
            pins[k].view(F32)[:] = xs[k]
            agg.submit(2, k, pins[k].view(F32), w[k], pinned=True)
            assert agg.progress(2) == (k + 1, 0)  # non-eager
        assert agg.host_read_kept(2) == 0
        submit_all(agg, 1, xs, w)
        submit_all(agg, 3, xs, w)
        agg.reduce_parts([1, 2, 3])
        assert (agg.noise_round(2), agg.noise_round(3)) == (1, 1)
        a = O.fedavg(xs, w)
        R.assert_bits(agg.finalize(1), a, "plain part of the batch")
        R.assert_bits(agg.finalize(2), N.noisy(a, stddev, SEED, 2, 0), "noise part of the batch")
        R.assert_bits(agg.finalize(3), R.round_out(N.noisy(a, stddev, SEED, 3, 0), "bf16"), "bf16 noise part of the batch")
        assert (agg.noise_round(2), agg.noise_round(3)) == (1, 1)  # the finalizes only copied out
        # fa_reduce_part twice: two rounds, two noises
        submit_all(agg, 2, xs, w)
        agg.reduce(2)
        agg.reduce(2)
        R.assert_bits(agg.copy_output(2), N.noisy(a, stddev, SEED, 2, 2), "second reducing call")
        assert agg.noise_round(2) == 3


# ------------------------------------------------------------------ refusals

def test_refusals(fa, O, torch_gpu):
    D, n = 3, 67
    w = O.weights(D)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.set_noise(1.0, SEED)
        assert e.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(e.value)
        agg.set_noise(0.0, 0)  # removing nothing is fine
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)
        with pytest.raises(fa.FaError) as e:
            agg.set_noise(1.0, SEED, 1)
        assert e.value.code == fa.ERR_ARG and "FA_LITERAL" in str(e.value)
        for bad in (-1.0, float("inf"), float("nan")):
            with pytest.raises(fa.FaError) as e:
                agg.set_noise(bad, SEED)
            assert e.value.code == fa.ERR_ARG and "stddev" in str(e.value)
        agg.set_noise(1.0, SEED)
        agg.define(2, n, fa.F32, fa.F32, D, mode=fa.LITERAL)  # ignores the context default
        assert agg.noise(2)[0] == 0.0
        agg.define(3, n, fa.F32, fa.F32, D)
        with pytest.raises(fa.FaError) as e:
            agg.set_noise_round(3, 2 ** 32 + 1)
        assert e.value.code == fa.ERR_ARG
        agg.set_noise_round(3, 2 ** 32 - 1)
        xs = make_clients(n, D, "f32", 71)
        submit_all(agg, 3, xs, w)
        R.assert_bits(agg.finalize(3), N.noisy(O.fedavg(xs, w), 1.0, SEED, 3, 2 ** 32 - 1), "the last round")
        assert agg.noise_round(3) == 2 ** 32
        submit_all(agg, 3, xs, w)
        with pytest.raises(fa.FaError) as e:  # the 2^32-th round
            agg.finalize(3)
        assert e.value.code == fa.ERR_STATE and "2^32" in str(e.value)
        agg.set_noise(1.0, SEED + 1, 3)
        agg.set_noise_round(3, 0)
        R.assert_bits(agg.finalize(3), N.noisy(O.fedavg(xs, w), 1.0, SEED + 1, 3, 0), "a new seed starts over")
