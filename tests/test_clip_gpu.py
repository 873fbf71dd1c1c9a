"""GPU: the clip stage (per-client L2 norm clipping, fa.h "Clip stage") against tests/clip_ref.py.

The stage's summation order is free, so a clipped round is checked by three independent assertions:
(a) every reported Q_k is within n * 2^-53 * exact of the exactly rounded sum (the bound fa.h derives for any
    order of fp64 adds of non-negative terms; NaN and inf must come back as NaN and inf),
(b) the reported scale and inclusion are bit-equal to rule 2 applied to the reported Q_k,
(c) the output is bit-equal to rules 3-4 (the oracle's FMA chain) computed from the reported scales.
Client k is g + sigma_k * noise with |noise| in [0.5, 1): sigma = 0.01 for even k and 0.5 for odd k against
C = 0.05 sqrt(n), so even clients pass and odd ones are clipped whatever the input rounding does (at most
2^-8 relative to |x| < 2 per element).  D = 1 has one client only: it is the clipped kind there.
"""
import numpy as np
import pytest

import clip_ref as R
import server_opt_ref as S

pytestmark = pytest.mark.gpu

F16, F32, F64, U16 = np.float16, np.float32, np.float64, np.uint16
SEED = 0xC11F
NS = [1, 7, 67, 4099, 100003]
DS = [1, 3, 8, 130]
KINDS = ["f32", "bf16", "f16"]


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def narrow(x, kind):
    """fp32 values as a receipt of `kind`."""
    return R.round_out(x, kind)


def bound_c(n):
    return float(F32(0.05 * np.sqrt(n)))


def sigma(k, D):
    return 0.5 if (k % 2 == 1 or D == 1) else 0.01


def make_ref(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(F32)


def make_clients(g, D, kind, seed):
    rng = np.random.default_rng(seed)
    xs = []
    for k in range(D):
        noise = rng.uniform(0.5, 1.0, g.size) * rng.choice([-1.0, 1.0], g.size)
        xs.append(narrow((g + F32(sigma(k, D)) * noise.astype(F32)).astype(F32), kind))
    return xs


def check_q(Q, xs, kind, g, what):
    """(a); returns the exact sums"""
    exacts = [R.sumsq(R.widen(x, kind), g) for x in xs]
    for k, exact in enumerate(exacts):
        if exact != exact:
            assert Q[k] != Q[k], (what, k, Q[k])
        elif exact == np.inf:
            assert Q[k] == np.inf, (what, k, Q[k])
        else:
            err, tol = abs(float(Q[k]) - exact), R.sumsq_bound(g.size, exact)
            assert err <= tol, "%s: Q[%d] = %r, exact %r, error %g > bound %g" % (what, k, Q[k], exact, err, tol)
    return exacts


def check_scales(Q, scales, included, C, what):
    """(b): an excluded client reports scale 0"""
    for k in range(len(Q)):
        s, inc = R.scale(Q[k], C)
        assert bool(included[k]) == inc and F32(scales[k]).view(np.uint32) == s.view(np.uint32), (what, k, Q[k], scales[k], s)


def check_round(agg, O, part, out, xs, kind, okind, w, g, C, what, expect_mix=True):
    """(a), (b), (c) for the round just reduced; returns the reported (Q, scales, included, n_clipped)."""
    Q, scales, included, n_clipped = agg.clip_round(part)
    exacts = check_q(Q, xs, kind, g, what)
    check_scales(Q, scales, included, C, what)
    assert n_clipped == int(np.sum(included & (scales < 1))), (what, n_clipped)
    if expect_mix:  # the case does clip someone, and (for D > 1) lets someone pass
        hs = [R.scale(q, C)[0] for q in exacts]
        assert any(s < 1 for s in hs) and (len(xs) == 1 or any(s == 1 for s in hs)), (what, hs)
    a = R.aggregate(O, xs, kind, w, scales, included, g)
    R.assert_bits(out, R.round_out(a, okind), what + " output")
    return Q, scales, included, n_clipped, a


def submit_all(agg, part, xs, w):
    for k, x in enumerate(xs):
        agg.submit(part, k, x, w[k])


# ------------------------------------------------------------------ the three assertions over sizes, D, dtypes

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_clipped_round_q_scales_and_output(fa, O, torch_gpu, D, kind):
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        for part, n in enumerate(NS, start=1):
            g = make_ref(n, SEED + n)
            xs = make_clients(g, D, kind, SEED + 7 * n + D)
            C = bound_c(n)
            agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
            agg.set_clip(C, part)
            agg.set_clip_reference(part, g)
            submit_all(agg, part, xs, w)
            out = agg.finalize(part)
            check_round(agg, O, part, out, xs, kind, kind, w, g, C, "%s D %d n %d" % (kind, D, n))
            R.assert_bits(agg.clip_reference(part), R.widen(out, kind), "reference := the output, widened")


def test_small_integers_are_exact(fa, O, torch_gpu):
    n, D = 5, 2
    g = np.asarray([1, -2, 3, 0, 7], F32)
    xs = [(g + np.asarray([3, 4, 0, 0, 0], F32)).astype(F32), g.copy()]
    w = np.asarray([0.25, 0.75], F32)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        for C, s0, clipped in ((5.0, 1.0, 0), (2.5, 0.5, 1)):
            agg.set_clip(C, 1)
            agg.set_clip_reference(1, g)
            submit_all(agg, 1, xs, w)
            out = agg.finalize(1)
            Q, scales, included, n_clipped, _ = check_round(agg, O, 1, out, xs, "f32", "f32", w, g, C, "C %g" % C,
                                                            expect_mix=False)
            assert Q.tolist() == [25.0, 0.0] and scales.tolist() == [s0, 1.0] and included.all() and n_clipped == clipped


# ------------------------------------------------------------------ raw entry

def dev_buf(torch, host, kind, offset):
    """host (a receipt of `kind`) on the device, `offset` elements into a fresh allocation."""
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.int16}[kind]
    t = torch.empty(host.size + 16, dtype=tdt, device="cuda")[offset:offset + host.size]
    src = host.view(np.int16) if kind == "bf16" else host
    t.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    return t


def raw_q(fa, torch, xs, kind, g, offsets, ref_offset, ctx=None):
    devs = [dev_buf(torch, x, kind, o) for x, o in zip(xs, offsets)]
    dg = dev_buf(torch, g, "f32", ref_offset)
    return fa.clip_sumsq_device(devs, g.size, fa_dt(fa, kind), dg, ctx=ctx)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_raw_entry_pointer_phases(fa, torch_gpu, kind):
    D = 3
    for n, offsets, ref_offset in ((4099, (1, 1, 1), 1),   # one shared phase: vector body, head and tail
                                   (4099, (0, 1, 2), 3),   # mixed phases: one element per lane
                                   (4099, (2, 2, 2), 3),   # the reference's phase alone is off
                                   (4099, (0, 0, 0), 0),
                                   (3, (1, 1, 1), 1)):     # shorter than the head
        g = make_ref(n, SEED + n)
        xs = make_clients(g, D, kind, SEED + 1)
        check_q(raw_q(fa, torch_gpu, xs, kind, g, offsets, ref_offset), xs, kind, g, "%s %s" % (kind, (n, offsets, ref_offset)))


def test_raw_entry_strided_tiles_and_determinism(fa, torch_gpu):
    """A grid capped below the tile count (25 tiles of 4096 elements on 3 workgroups), and the same call twice."""
    n, D = 100003, 3
    g = make_ref(n, SEED)
    xs = make_clients(g, D, "f32", SEED + 2)
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=3)
        q1 = raw_q(fa, torch_gpu, xs, "f32", g, (0, 0, 0), 0, ctx=agg)
        check_q(q1, xs, "f32", g, "3 workgroups")
    devs = [dev_buf(torch_gpu, x, "f32", 0) for x in xs]
    dg = dev_buf(torch_gpu, g, "f32", 0)
    a = fa.clip_sumsq_device(devs, n, fa.F32, dg)
    b = fa.clip_sumsq_device(devs, n, fa.F32, dg)
    check_q(a, xs, "f32", g, "one-shot grid")
    assert a.view(np.uint64).tolist() == b.view(np.uint64).tolist()


# ------------------------------------------------------------------ specials

def test_nan_inf_and_huge_clients(fa, O, torch_gpu):
    n, D = 4099, 5
    g = make_ref(n, SEED)
    xs = make_clients(g, D, "f32", SEED + 3)
    xs[0][17] = np.nan
    xs[1][4000] = np.inf
    xs[2][:] = F32(1e30)
    w = O.weights(D)
    C = bound_c(n)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_clip(C, 1)
        agg.set_clip_reference(1, g)
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        Q, scales, included, n_clipped, _ = check_round(agg, O, 1, out, xs, "f32", "f32", w, g, C, "specials")
        assert included.tolist() == [False, False, True, True, True] and scales[0] == 0 and scales[1] == 0
        assert 0 < scales[2] < 1e-25 and np.isfinite(out).all()


def test_reference_holding_an_inf_excludes_everyone(fa, O, torch_gpu):
    n, D = 4099, 3
    g = make_ref(n, SEED)
    xs = make_clients(g, D, "f32", SEED + 4)
    g[100] = np.inf
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_clip(1.0, 1)
        agg.set_clip_reference(1, g)
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        Q, scales, included, n_clipped, _ = check_round(agg, O, 1, out, xs, "f32", "f32", w, g, 1.0, "inf reference",
                                                        expect_mix=False)
        assert not included.any() and n_clipped == 0 and out[100] == np.inf and np.isfinite(np.delete(out, 100)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_a_huge_bound_is_plain_fedavg(fa, O, torch_gpu, kind):
    n, D = 4099, 8
    g = make_ref(n, SEED)
    xs = make_clients(g, D, kind, SEED + 5)
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.define(2, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.set_clip(1e30, 1)
        agg.set_clip_reference(1, g)
        submit_all(agg, 1, xs, w)
        submit_all(agg, 2, xs, w)
        out = agg.finalize(1)
        R.assert_bits(out, agg.finalize(2), "unclipped round == plain FedAvg")
        Q, scales, included, n_clipped = agg.clip_round(1)
        assert n_clipped == 0 and included.all() and (scales == 1).all()
        check_q(Q, xs, kind, g, "huge bound")


# ------------------------------------------------------------------ through a context

def rounds_on(fa, O, agg, part, D, n, kind, okind, C, rounds=("finalize", "finalize", "reduce"), what=""):
    """The bootstrap round and clipped rounds after it, each reduced the way `rounds` names; returns the last
    reference.  Round r's receipts surround the reference the round before left."""
    w = O.weights(D)
    g = None
    for r, how in enumerate(rounds):
        base = make_ref(n, SEED + 100) if g is None else g
        xs = make_clients(base, D, kind, SEED + 31 * r + D)
        submit_all(agg, part, xs, w)
        if how == "finalize":
            out = agg.finalize(part)
        elif how == "reduce_parts":
            agg.reduce_parts([part])
            out = agg.finalize(part)  # only copies out
        else:
            agg.reduce(part)
            out = agg.copy_output(part)
        tag = "%s round %d by %s" % (what, r + 1, how)
        if g is None:  # the bootstrap: the plain aggregate, reported as unclipped
            Q, scales, included, n_clipped = agg.clip_round(part)
            assert not Q.any() and (scales == 1).all() and included.all() and n_clipped == 0, tag
            a = R.aggregate(O, xs, kind, w, scales, included, np.zeros(n, F32))
            R.assert_bits(out, R.round_out(a, okind), tag + " output")
        else:
            check_round(agg, O, part, out, xs, kind, okind, w, g, C, tag)
        g = R.widen(out, okind)
        R.assert_bits(agg.clip_reference(part), g, tag + " reference")
    return g


@pytest.mark.parametrize("kind,okind", [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("f32", "bf16"), ("f16", "f32")])
def test_context_bootstrap_then_clipped_rounds(fa, O, torch_gpu, kind, okind):
    D, n = 3, 4099
    with fa.Aggregator(1) as agg:
        agg.set_clip(bound_c(n))  # the context default: FedAvg parts defined later take it
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, okind), D)
        with pytest.raises(fa.FaError) as e:  # no reference before the first round
            agg.clip_reference(1)
        assert e.value.code == fa.ERR_STATE
        rounds_on(fa, O, agg, 1, D, n, kind, okind, bound_c(n), rounds=("finalize", "finalize", "reduce", "reduce_parts"))


def test_two_range_shards(fa, O, torch_gpu):
    D, n = 3, 100003
    with fa.Aggregator(devices=[0, 0], shared_device=True) as agg:
        agg.set_clip(bound_c(n))
        agg.define(1, n, fa.F32, fa.F32, D)
        rounds_on(fa, O, agg, 1, D, n, "f32", "f32", bound_c(n), what="two shards")
        g = make_ref(n, 5)  # scattered to the shards, gathered back
        agg.set_clip_reference(1, g)
        R.assert_bits(agg.clip_reference(1), g, "reference round trip")


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_range_pieces(fa, O, torch_gpu, kind):
    D, n = 5, 100003
    with fa.Aggregator(1) as agg:
        agg.set_tuning(piece_span_kib=512, piece_split_kib=-1)
        agg.set_clip(bound_c(n))
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        assert len(agg.pieces(1, 0, 0)) >= 2
        rounds_on(fa, O, agg, 1, D, n, kind, kind, bound_c(n), what="pieces")


def test_reduce_parts_mixes_a_clipped_and_a_plain_part(fa, O, torch_gpu):
    D, n = 3, 4099
    w = O.weights(D)
    C = bound_c(n)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_clip(C, 1)
        g = make_ref(n, SEED)
        agg.set_clip_reference(1, g)
        xs = make_clients(g, D, "f32", SEED + 6)
        agg.submit(1, 0, xs[0], w[0])
        with pytest.raises(fa.FaError) as e:  # a clipped part needs every client
            agg.reduce_parts([1, 2], weights=[w, w])
        assert e.value.code == fa.ERR_STATE
        submit_all(agg, 1, xs, w)
        submit_all(agg, 2, xs, w)
        agg.reduce_parts([1, 2])
        check_round(agg, O, 1, agg.finalize(1), xs, "f32", "f32", w, g, C, "clipped part of a batch")
        R.assert_bits(agg.finalize(2), O.fedavg(xs, w), "plain part of the batch")
        with pytest.raises(fa.FaError) as e:
            agg.clip_round(2)
        assert e.value.code == fa.ERR_STATE


def test_reference_set_dropped_and_stage_removed(fa, O, torch_gpu):
    D, n = 3, 4099
    w = O.weights(D)
    C = bound_c(n)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        with pytest.raises(fa.FaError) as e:
            agg.set_clip_reference(1, np.zeros(n, F32))
        assert e.value.code == fa.ERR_STATE
        agg.set_clip(C, 1)
        g = make_ref(n, SEED)
        agg.set_clip_reference(1, g)
        R.assert_bits(agg.clip_reference(1), g, "round trip")
        agg.set_clip(2 * C, 1)  # the bound changes, the reference stays
        R.assert_bits(agg.clip_reference(1), g, "kept over a new bound")
        agg.set_clip_reference(1, None)  # dropped: the next round bootstraps
        with pytest.raises(fa.FaError) as e:
            agg.clip_reference(1)
        assert e.value.code == fa.ERR_STATE
        xs = make_clients(g, D, "f32", SEED + 8)
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        R.assert_bits(out, O.fedavg(xs, w), "bootstrap after the drop")
        assert agg.clip_round(1)[3] == 0
        R.assert_bits(agg.clip_reference(1), out, "reference from the bootstrap")
        agg.set_clip(0.0, 1)  # removed: plain FedAvg, no stage state
        submit_all(agg, 1, xs, w)
        R.assert_bits(agg.finalize(1), O.fedavg(xs, w), "stage removed")
        with pytest.raises(fa.FaError) as e:
            agg.clip_round(1)
        assert e.value.code == fa.ERR_STATE


@pytest.mark.parametrize("order", ["opt first", "clip first"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_clipped_aggregate_feeds_the_server_optimizer(fa, O, torch_gpu, kind, order):
    D, n = 3, 4099
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    w = O.weights(D)
    C = bound_c(n)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        if order == "opt first":
            agg.set_server_opt(S.ADAM, part_id=1, **hp)
            agg.set_clip(C, 1)
        else:
            agg.set_clip(C, 1)
            agg.set_server_opt(S.ADAM, part_id=1, **hp)
        x0 = make_ref(n, SEED + 9)
        agg.set_server_opt_state(1, x=x0)
        g = R.widen(narrow(x0, kind), kind)  # what the owners hold: the master in the bucket's dtype
        agg.set_clip_reference(1, g)
        ref = (x0, np.zeros(n, F32), np.zeros(n, F32))
        for step in (1, 2):
            xs = make_clients(g, D, kind, SEED + 40 + step)
            submit_all(agg, 1, xs, w)
            out = agg.finalize(1)
            Q, scales, included, n_clipped = agg.clip_round(1)
            check_q(Q, xs, kind, g, "step %d" % step)
            check_scales(Q, scales, included, C, "step %d" % step)
            assert 0 < n_clipped < D
            ref = S.step(S.ADAM, R.aggregate(O, xs, kind, w, scales, included, g), *ref, **hp)
            x, m, v, k = agg.server_opt_state(1)
            assert k == step
            for got, exp, name in ((x, ref[0], "x"), (m, ref[1], "m"), (v, ref[2], "v")):
                R.assert_bits(got, exp, "%s %s step %d %s" % (kind, order, step, name))
            R.assert_bits(out, S.round_out(ref[0], kind), "step %d output" % step)
            g = R.widen(out, kind)
            R.assert_bits(agg.clip_reference(1), g, "step %d reference" % step)


def test_refusals_and_an_eager_context(fa, O, torch_gpu):
    D, n = 3, 67
    w = O.weights(D)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.set_clip(1.0)
        assert e.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(e.value)
    with fa.Aggregator(1, eager=True) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)
        agg.define(2, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        for part, name in ((1, "FA_LITERAL"), (2, "FA_TRIMMED")):
            with pytest.raises(fa.FaError) as e:
                agg.set_clip(1.0, part)
            assert e.value.code == fa.ERR_ARG and name in str(e.value)
        with pytest.raises(fa.FaError) as e:
            agg.set_clip(-1.0)
        assert e.value.code == fa.ERR_ARG and "max_norm" in str(e.value)
        agg.set_clip(bound_c(n))
        agg.define(3, n, fa.F32, fa.F32, D)  # takes the context's bound: non-eager, never kept host-side
        g = make_ref(n, SEED)
        agg.set_clip_reference(3, g)
        xs = make_clients(g, D, "f32", SEED + 10)
        pins = [fa.PinnedBuffer(n * 4) for _ in range(D)]
        for k in range(D):
            pins[k].view(F32)[:] = xs[k]
            agg.submit(3, k, pins[k].view(F32), w[k], pinned=True)
            assert agg.progress(3) == (k + 1, 0)
        assert agg.host_read_kept(3) == 0
        check_round(agg, O, 3, agg.finalize(3), xs, "f32", "f32", w, g, bound_c(n), "eager context")
