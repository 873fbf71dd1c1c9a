"""GPU: the Krum stage (Krum / Multi-Krum selection over pairwise distances, fa.h "Krum stage") against
tests/krum_ref.py.

The distance pass's summation order is free, so a round is checked by four independent assertions:
(a) every reported Q_ab is within n * 2^-53 * exact of the exactly rounded sum (the bound fa.h derives for any
    order of fp64 adds of non-negative terms; NaN and inf must come back as NaN and inf), the matrix is
    bit-symmetric and its diagonal is +0,
(b) the reported scores and selection are bit-equal to rules 2-3 applied to the reported matrix,
(c) the output is bit-equal to rules 4-5 (the oracle's FMA chain) computed from the reported selection,
(d) the selection is the one the data were built for, so the test cannot pass by agreeing with itself.
Client k is g + sigma_k * noise with |noise| in [0.5, 1): sigma = 8 for the f Byzantine clients, the odd indices
1, 3, ..., 2f - 1, and 0.01 for the honest rest, rounded to the input dtype (bf16 is the coarsest: at most
0.0313 off below 16, 0.0039 off below 2).  Two honest clients are then at most 0.02 + 0.0078 apart per element
(q <= 7.8e-4), a Byzantine one at least 4 - 0.01 - 0.0352 from any honest one (q >= 15.6).  A score has
D - f - 2 terms.  An honest client has D - f - 1 honest neighbours, so its score is at most (D - f - 2) 7.8e-4 n
<= 0.05 n.  A Byzantine client has only f - 1 Byzantine neighbours (which may lie close to it), so at least
D - 2f - 1 >= 2 of its terms are distances to honest clients: its score is at least 31.2 n, more than 600 times
any honest score.  The exact rule therefore selects exactly the honest set for m = D - f and an honest client
for m = 1, and the n * 2^-53 freedom of the sums cannot move the selection.

The exact reference costs D^2 n / 2 on the host.  For D = 128 at n = 100003 (8128 pairs) assertion (a) runs on a
fixed sample of 256 pairs; everything else, and every other shape, is checked in full.
"""
import numpy as np
import pytest

import krum_ref as K
import server_opt_ref as S
from guarded import GuardedBuf, assert_unchanged, snapshot

pytestmark = pytest.mark.gpu

F16, F32, F64, U16 = np.float16, np.float32, np.float64, np.uint16
SEED = 0xC2A5
NS = [1, 7, 67, 4099, 100003]
DF = [(3, 0), (4, 0), (5, 1), (8, 2), (33, 10), (128, 62)]
KINDS = ["f32", "bf16", "f16"]
SAMPLE_ABOVE = 200_000_000  # pair-elements (D (D-1) / 2 * n) above which (a) samples 256 pairs


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def byzantine(D, f):
    return [k for k in range(D) if k % 2 == 1 and k < 2 * f]


def honest_flags(D, f):
    sel = np.ones(D, bool)
    sel[byzantine(D, f)] = False
    return sel


def make_clients(n, D, f, kind, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, n).astype(F32)
    bad = set(byzantine(D, f))
    xs = []
    for k in range(D):
        noise = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
        xs.append(K.round_out((g + F32(8.0 if k in bad else 0.01) * noise.astype(F32)).astype(F32), kind))
    return xs


def bits64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def check_q(Q, xs, kind, what):
    """(a)"""
    D = len(xs)
    n = np.asarray(xs[0]).size
    assert Q.shape == (D, D) and np.array_equal(bits64(Q), bits64(Q.T)), what + ": not bit-symmetric"
    assert not bits64(np.diag(Q)).any(), what + ": the diagonal is not +0"
    ws = [K.widen(x, kind) for x in xs]
    pairs = [(a, b) for a in range(D) for b in range(a + 1, D)]
    if len(pairs) * n > SAMPLE_ABOVE:
        pick = np.random.default_rng(SEED).choice(len(pairs), 256, replace=False)
        pairs = [pairs[i] for i in sorted(pick)]
    for a, b in pairs:
        exact = K.pair_sumsq(ws[a], ws[b])
        if exact != exact:
            assert Q[a, b] != Q[a, b], (what, a, b, Q[a, b])
        elif exact == np.inf:
            assert Q[a, b] == np.inf, (what, a, b, Q[a, b])
        else:
            err, tol = abs(float(Q[a, b]) - exact), K.dist_bound(n, exact)
            assert err <= tol, "%s: Q[%d, %d] = %r, exact %r, error %g > bound %g" % (what, a, b, Q[a, b], exact, err, tol)


def check_round(agg, O, part, out, xs, kind, okind, w, f, m, what, expect=None):
    """(a), (b), (c) and, with `expect`, (d) for the round just reduced; returns (Q, scores, selected, aggregate)."""
    Q, scores, sel = agg.krum_round(part)
    check_q(Q, xs, kind, what)
    rS, rsel = K.krum_select(Q, f, m)
    assert np.array_equal(bits64(scores), bits64(rS)), (what, scores, rS)
    assert sel.tolist() == rsel.tolist(), (what, sel, rsel)
    a = K.aggregate(O, xs, kind, w, sel)
    K.assert_bits(out, K.round_out(a, okind), what + " output")
    if expect is not None:
        assert sel.tolist() == list(expect), (what, sel)
    return Q, scores, sel, a


def submit_all(agg, part, xs, w):
    for k, x in enumerate(xs):
        agg.submit(part, k, x, w[k])


# ------------------------------------------------------------------ the four assertions over sizes, D, dtypes

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,f", DF)
def test_multi_krum_and_krum_rounds(fa, O, torch_gpu, D, f, kind):
    w = O.weights(D)
    honest = honest_flags(D, f)
    with fa.Aggregator(1) as agg:
        for part, n in enumerate(NS, start=1):
            xs = make_clients(n, D, f, kind, SEED + 7 * n + D)
            agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
            agg.set_krum(f, None, part)  # Multi-Krum, m = D - f: exactly the honest set
            submit_all(agg, part, xs, w)
            out = agg.finalize(part)
            what = "%s D %d f %d n %d" % (kind, D, f, n)
            Q, scores, sel, _ = check_round(agg, O, part, out, xs, kind, kind, w, f, D - f, what, expect=honest)
            if f:
                assert scores[~honest].min() > 600 * scores[honest].max(), (what, scores)
            if n == 100003 and D * (D - 1) // 2 * n > SAMPLE_ABOVE:
                continue  # one exact sample of this shape is enough
            agg.set_krum(f, 1, part)  # Krum, m = 1: one honest client
            submit_all(agg, part, xs, w)
            out = agg.finalize(part)
            Q1, _, sel1, _ = check_round(agg, O, part, out, xs, kind, kind, w, f, 1, what + " m 1")
            assert sel1.sum() == 1 and honest[np.flatnonzero(sel1)[0]], (what, sel1)
            assert np.array_equal(bits64(Q1), bits64(Q)), what + ": the same layout gave other bits"


def test_small_integers_are_exact(fa, O, torch_gpu):
    n, D = 5, 3
    g = np.asarray([1, -2, 3, 0, 7], F32)
    xs = [(g + np.asarray([3, 4, 0, 0, 0], F32)).astype(F32), g.copy(), (g + np.asarray([0, 0, 0, 12, 5], F32)).astype(F32)]
    w = np.asarray([0.25, 0.5, 0.25], F32)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_krum(0, 1, 1)
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        Q, scores, sel, _ = check_round(agg, O, 1, out, xs, "f32", "f32", w, 0, 1, "3-4-5")
        assert Q.tolist() == [[0.0, 25.0, 194.0], [25.0, 0.0, 169.0], [194.0, 169.0, 0.0]]  # 9 + 16 + 144 + 25
        assert scores.tolist() == [25.0, 25.0, 169.0] and sel.tolist() == [True, False, False]  # the tie: lower index
        # m = 1 keeps the round's mass: w'_0 = w_0 W / w_0 = 1 here, so the reply is fl32(1 x_0 + 0)
        K.assert_bits(out, O.fedavg([xs[0]], np.asarray([1.0], F32)), "the chosen owner's bucket times W")


def test_two_identical_clients(fa, O, torch_gpu):
    n, D = 4099, 4
    xs = make_clients(n, D, 0, "f32", SEED + 1)
    xs[3] = xs[1].copy()
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_krum(0, 1, 1)
        submit_all(agg, 1, xs, w)
        Q, scores, sel, _ = check_round(agg, O, 1, agg.finalize(1), xs, "f32", "f32", w, 0, 1, "twins")
        assert bits64(Q[1, 3]) == 0 and scores[1] == scores[3] and sel.tolist() == [False, True, False, False]


@pytest.mark.parametrize("poison", ["nan", "inf", "1e30"])
def test_a_poisoned_client_is_left_out(fa, O, torch_gpu, poison):
    n, D, f = 4099, 5, 1
    xs = make_clients(n, D, 0, "f32", SEED + 2)  # everyone honest, then client 2 is poisoned
    xs[2][:] = {"nan": np.nan, "inf": np.inf, "1e30": F32(1e30)}[poison]
    w = O.weights(D)
    expect = [True, True, False, True, True]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_krum(f, None, 1)
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        Q, scores, sel, _ = check_round(agg, O, 1, out, xs, "f32", "f32", w, f, D - f, poison, expect=expect)
        assert np.isfinite(out).all()
        row = np.delete(Q[2], 2)
        if poison == "nan":
            assert np.isnan(row).all() and bits64(Q[2, 2]) == 0 and scores[2] == np.inf
        elif poison == "inf":
            assert (row == np.inf).all() and scores[2] == np.inf
        else:
            assert np.isfinite(row).all() and (row > 1e60).all() and np.isfinite(scores[2])


@pytest.mark.parametrize("kind", KINDS)
def test_f_0_and_m_D_is_plain_fedavg(fa, O, torch_gpu, kind):
    n, D = 4099, 8
    xs = make_clients(n, D, 2, kind, SEED + 3)
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.define(2, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.set_krum(0, D, 1)
        submit_all(agg, 1, xs, w)
        submit_all(agg, 2, xs, w)
        out = agg.finalize(1)
        K.assert_bits(out, agg.finalize(2), "nobody deselected == plain FedAvg")
        Q, scores, sel = agg.krum_round(1)
        assert sel.all()
        check_q(Q, xs, kind, "f 0 m D")
        agg.set_krum(0, 0, 1)  # removed: plain FedAvg, no stage state
        submit_all(agg, 1, xs, w)
        K.assert_bits(agg.finalize(1), out, "stage removed")
        with pytest.raises(fa.FaError) as e:
            agg.krum_round(1)
        assert e.value.code == fa.ERR_STATE


# ------------------------------------------------------------------ raw entry

def guarded_clients(torch, xs, kind, offsets):
    """The receipts in GuardedBufs at the given 16-byte phases (in elements): (bufs, typed views, snapshots)."""
    item = 4 if kind == "f32" else 2
    tdt = torch.int32 if kind == "f32" else torch.int16
    bufs, views, snaps = [], [], []
    for x, o in zip(xs, offsets):
        b = GuardedBuf(torch, x.size * item, o * item)
        v = b.view(tdt)
        v.copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if kind == "f32" else np.int16)))
        bufs.append(b)
        views.append(v)
        snaps.append(snapshot(v))
    torch.cuda.synchronize()
    return bufs, views, snaps


@pytest.mark.parametrize("kind", KINDS)
def test_raw_entry_pointer_phases_in_guarded_buffers(fa, torch_gpu, kind):
    D = 5
    for n, offsets in ((4099, (1, 1, 1, 1, 1)),   # one shared phase: vector body, head and tail
                       (4099, (0, 1, 2, 3, 0)),   # mixed phases: the element form
                       (4099, (0, 0, 0, 0, 0)),
                       (100003, (3, 0, 1, 2, 3)),  # the element form over several workgroups
                       (3, (1, 1, 1, 1, 1))):     # shorter than the head
        xs = make_clients(n, D, 1, kind, SEED + n)
        bufs, views, snaps = guarded_clients(torch_gpu, xs, kind, offsets)
        Q = fa.pairdist_device([b.ptr for b in bufs], n, fa_dt(fa, kind))
        what = "%s %s" % (kind, (n, offsets))
        check_q(Q, xs, kind, what)
        for k in range(D):
            bufs[k].check(what + " client %d" % k)
            assert_unchanged(views[k], snaps[k], what + " client %d" % k)


def test_raw_entry_strided_tiles_and_determinism(fa, torch_gpu):
    """A grid capped below the tile count (98 tiles of 1024 elements on 3 workgroups), and the same call twice."""
    n, D = 100003, 8
    xs = make_clients(n, D, 2, "f32", SEED + 4)
    bufs, views, snaps = guarded_clients(torch_gpu, xs, "f32", [0] * D)
    ptrs = [b.ptr for b in bufs]
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=3)
        check_q(fa.pairdist_device(ptrs, n, fa.F32, ctx=agg), xs, "f32", "3 workgroups")
    a = fa.pairdist_device(ptrs, n, fa.F32)
    b = fa.pairdist_device(ptrs, n, fa.F32)
    check_q(a, xs, "f32", "one-shot grid")
    assert np.array_equal(bits64(a), bits64(b))
    for k in range(D):
        bufs[k].check("client %d" % k)
        assert_unchanged(views[k], snaps[k], "client %d" % k)


def test_raw_entry_one_and_two_clients(fa, torch_gpu):
    n = 4099
    xs = make_clients(n, 2, 0, "f32", SEED + 5)
    bufs, _, _ = guarded_clients(torch_gpu, xs, "f32", [0, 0])
    assert bits64(fa.pairdist_device([bufs[0].ptr], n, fa.F32)).tolist() == [[0]]
    check_q(fa.pairdist_device([b.ptr for b in bufs], n, fa.F32), xs, "f32", "D 2")


# ------------------------------------------------------------------ through a context

def one_gpu_round(fa, O, xs, kind, w, f, m):
    D, n = len(xs), np.asarray(xs[0]).size
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.set_krum(f, m, 1)
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        return out, agg.krum_round(1)


def test_two_range_shards_match_one_gpu(fa, O, torch_gpu):
    D, f, n = 5, 1, 100003
    xs = make_clients(n, D, f, "f32", SEED + 6)
    w = O.weights(D)
    ref_out, (_, _, ref_sel) = one_gpu_round(fa, O, xs, "f32", w, f, None)
    with fa.Aggregator(devices=[0, 0], shared_device=True) as agg:
        agg.set_krum(f)  # the context default: FedAvg parts defined later take it
        agg.define(1, n, fa.F32, fa.F32, D)
        for how in ("finalize", "reduce", "reduce_parts"):
            submit_all(agg, 1, xs, w)
            if how == "finalize":
                out = agg.finalize(1)
            elif how == "reduce":
                agg.reduce(1)
                out = agg.copy_output(1)
            else:
                agg.reduce_parts([1])
                out = agg.finalize(1)  # only copies out
            _, _, sel, _ = check_round(agg, O, 1, out, xs, "f32", "f32", w, f, D - f, "two shards by " + how,
                                       expect=honest_flags(D, f))
            assert sel.tolist() == ref_sel.tolist()
            K.assert_bits(out, ref_out, "two shards == one GPU, by " + how)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_range_pieces_match_one_piece(fa, O, torch_gpu, kind):
    D, f, n = 5, 1, 100003
    xs = make_clients(n, D, f, kind, SEED + 7)
    w = O.weights(D)
    ref_out, (_, _, ref_sel) = one_gpu_round(fa, O, xs, kind, w, f, None)
    with fa.Aggregator(1) as agg:
        agg.set_tuning(piece_span_kib=512, piece_split_kib=-1)
        agg.set_krum(f)
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        assert len(agg.pieces(1, 0, 0)) >= 2
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        _, _, sel, _ = check_round(agg, O, 1, out, xs, kind, kind, w, f, D - f, "pieces", expect=honest_flags(D, f))
        assert sel.tolist() == ref_sel.tolist()
        K.assert_bits(out, ref_out, "pieces == one piece")


@pytest.mark.parametrize("order", ["opt first", "krum first"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_krum_aggregate_feeds_the_server_optimizer(fa, O, torch_gpu, kind, order):
    D, f, n = 5, 1, 4099
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        if order == "opt first":
            agg.set_server_opt(S.ADAM, part_id=1, **hp)
            agg.set_krum(f, None, 1)
        else:
            agg.set_krum(f, None, 1)
            agg.set_server_opt(S.ADAM, part_id=1, **hp)
        x0 = np.random.default_rng(SEED + 9).uniform(-1, 1, n).astype(F32)
        agg.set_server_opt_state(1, x=x0)
        ref = (x0, np.zeros(n, F32), np.zeros(n, F32))
        for step in (1, 2):
            xs = make_clients(n, D, f, kind, SEED + 40 + step)
            submit_all(agg, 1, xs, w)
            out = agg.finalize(1)
            Q, scores, sel = agg.krum_round(1)
            check_q(Q, xs, kind, "step %d" % step)
            assert sel.tolist() == honest_flags(D, f).tolist()
            ref = S.step(S.ADAM, K.aggregate(O, xs, kind, w, sel), *ref, **hp)
            x, m, v, k = agg.server_opt_state(1)
            assert k == step
            for got, exp, name in ((x, ref[0], "x"), (m, ref[1], "m"), (v, ref[2], "v")):
                K.assert_bits(got, exp, "%s %s step %d %s" % (kind, order, step, name))
            K.assert_bits(out, S.round_out(ref[0], kind), "step %d output" % step)


def test_reduce_parts_mixes_a_krum_and_a_plain_part_and_needs_every_client(fa, O, torch_gpu):
    D, f, n = 5, 1, 4099
    w = O.weights(D)
    xs = make_clients(n, D, f, "f32", SEED + 10)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_krum(f, None, 1)
        agg.submit(1, 0, xs[0], w[0])
        with pytest.raises(fa.FaError) as e:  # a Krum part needs every client
            agg.reduce_parts([1, 2], weights=[w, w])
        assert e.value.code == fa.ERR_STATE
        with pytest.raises(fa.FaError) as e:
            agg.reduce(1, weights=w)
        assert e.value.code == fa.ERR_STATE
        with pytest.raises(fa.FaError) as e:
            agg.krum_round(1)  # never reduced with the stage
        assert e.value.code == fa.ERR_STATE
        submit_all(agg, 1, xs, w)
        submit_all(agg, 2, xs, w)
        agg.reduce_parts([1, 2])
        check_round(agg, O, 1, agg.finalize(1), xs, "f32", "f32", w, f, D - f, "Krum part of a batch",
                    expect=honest_flags(D, f))
        K.assert_bits(agg.finalize(2), O.fedavg(xs, w), "plain part of the batch")
        with pytest.raises(fa.FaError) as e:
            agg.krum_round(2)
        assert e.value.code == fa.ERR_STATE


def test_refusals_and_an_eager_context(fa, O, torch_gpu):
    D, n = 5, 67
    w = O.weights(D)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.set_krum(1)
        assert e.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(e.value)
    with fa.Aggregator(1, eager=True) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)
        agg.define(2, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        for part, name in ((1, "FA_LITERAL"), (2, "FA_TRIMMED")):
            with pytest.raises(fa.FaError) as e:
                agg.set_krum(1, None, part)
            assert e.value.code == fa.ERR_ARG and name in str(e.value)
        agg.define(3, n, fa.F32, fa.F32, D)
        for f, m, says in ((2, None, "f = 2"), (-1, None, "f = -1"), (1, 5, "m = 5"), (1, -2, "m = -2")):
            with pytest.raises(fa.FaError) as e:
                agg.set_krum(f, m, 3)
            assert e.value.code == fa.ERR_ARG and says in str(e.value)
        agg.set_krum(1, None, 3)
        with pytest.raises(fa.FaError) as e:  # set_clip after set_krum
            agg.set_clip(1.0, 3)
        assert e.value.code == fa.ERR_ARG and "Krum" in str(e.value)
        agg.define(4, n, fa.F32, fa.F32, D)
        agg.set_clip(1.0, 4)
        with pytest.raises(fa.FaError) as e:  # set_krum after set_clip
            agg.set_krum(1, None, 4)
        assert e.value.code == fa.ERR_ARG and "clip" in str(e.value)
        agg.set_krum(1)  # the context default
        with pytest.raises(fa.FaError) as e:
            agg.set_clip(1.0)
        assert e.value.code == fa.ERR_ARG and "Krum" in str(e.value)
        with pytest.raises(fa.FaError) as e:  # checked against D at define time
            agg.define(5, n, fa.F32, fa.F32, 4)
        assert e.value.code == fa.ERR_ARG and "f = 1" in str(e.value)
        agg.define(5, n, fa.F32, fa.F32, D)  # takes the context's stage: non-eager, never kept host-side
        xs = make_clients(n, D, 1, "f32", SEED + 11)
        pins = [fa.PinnedBuffer(n * 4) for _ in range(D)]
        for k in range(D):
            pins[k].view(F32)[:] = xs[k]
            agg.submit(5, k, pins[k].view(F32), w[k], pinned=True)
            assert agg.progress(5) == (k + 1, 0)
        assert agg.host_read_kept(5) == 0
        check_round(agg, O, 5, agg.finalize(5), xs, "f32", "f32", w, 1, D - 1, "eager context", expect=honest_flags(D, 1))
