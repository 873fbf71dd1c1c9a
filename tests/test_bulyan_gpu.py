"""GPU: the Bulyan stage (iterated Krum, then a median-centred mean; fa.h "Bulyan stage") through an Aggregator,
against tests/bulyan_ref.py.

The distance pass's summation order is free, so a round is checked by four independent assertions, as in
tests/test_krum_gpu.py:
(a) every reported Q_ab is within n * 2^-53 * exact of the exactly rounded sum, the matrix is bit-symmetric and
    its diagonal is +0,
(b) the reported pick order and pick scores are bit-equal to rule 2 applied to the reported matrix,
(c) the output is bit-equal to rules 3-4 computed from the reported selection,
(d) exactly theta = D - 2f owners are picked and none of them is Byzantine, so the test cannot pass by agreeing
    with itself.
Honest owners hold g + 0.01 noise with |noise| in [0.5, 1); the b-th Byzantine owner (the odd indices 1, 3, ...,
2f - 1) holds g + 8 (b + 1) e with e = +-1 per element, all rounded to the input dtype (bf16 the coarsest: at most
0.5 off below 256, 0.0039 off below 2).  Per element two honest owners are at most 0.02 + 0.0078 apart
(q <= 7.8e-4), a Byzantine owner at least 8 - 0.5 - 0.01 - 0.0039 from an honest one and two Byzantine owners at
least 8 - 1 from each other (q >= 47 in both cases).  While only honest owners have been picked, p < theta of
them, R holds the f Byzantine owners and D - f - p honest ones, and c = max(1, D - f - p - 2).  A Byzantine
owner's score has at least one term and every term is a distance of 47 n or more.  An honest owner has
D - f - p - 1 >= c honest neighbours in R (for f >= 1, D - f - p >= f + 1 >= 2; for f = 0 there is no Byzantine
owner), so its score is at most c 7.8e-4 n <= 0.1 n.  By induction the rule picks honest owners only, and the
n * 2^-53 freedom of the sums cannot change that.

The exact matrix costs D^2 n / 2 on the host: it is computed once per (D, f, input kind, n) and shared.
"""
import functools

import numpy as np
import pytest

import bulyan_ref as B
import krum_ref as K
import noise_ref as N
import server_opt_ref as S
import trimmed_ref as T
from guarded import PAIRS

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = 0xB01A
NS = [1, 7, 67, 4099]
DF = [(3, 0), (7, 1), (8, 1), (11, 2), (33, 7), (67, 16), (128, 31)]


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def byzantine(D, f):
    return [k for k in range(D) if k % 2 == 1 and k < 2 * f]


def make_clients(n, D, f, kind, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, n).astype(F32)
    bad = byzantine(D, f)
    xs = []
    for k in range(D):
        if k in bad:
            e = rng.choice([-1.0, 1.0], n).astype(F32)
            xs.append(K.round_out((g + F32(8.0 * (bad.index(k) + 1)) * e).astype(F32), kind))
        else:
            noise = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
            xs.append(K.round_out((g + F32(0.01) * noise.astype(F32)).astype(F32), kind))
    return xs


@functools.lru_cache(maxsize=None)
def case(D, f, kind, n):
    """(the receipts, the exact matrix) of one shape, shared by the out dtypes."""
    xs = make_clients(n, D, f, kind, SEED + 7 * n + D)
    return xs, K.distances(xs, kind)


def bits64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def check_q(Q, exact, n, what):
    """(a)"""
    D = exact.shape[0]
    assert Q.shape == (D, D) and np.array_equal(bits64(Q), bits64(Q.T)), what + ": not bit-symmetric"
    assert not bits64(np.diag(Q)).any(), what + ": the diagonal is not +0"
    nan = np.isnan(exact)
    assert np.array_equal(np.isnan(Q), nan), what + ": NaN entries differ"
    inf = exact == np.inf
    assert np.array_equal(Q == np.inf, inf), what + ": inf entries differ"
    ok = ~(nan | inf)
    err, tol = np.abs(Q[ok] - exact[ok]), K.dist_bound(n, exact[ok])
    assert (err <= tol).all(), "%s: a distance is %g off, bound %g" % (what, (err - tol).max(), tol[np.argmax(err - tol)])


def check_round(agg, part, out, xs, exact, kind, okind, f, what, honest_only=True, a_of=None):
    """(a), (b), (c) and (d) for the round just reduced; returns (Q, order, selected, the fp32 aggregate).  a_of:
    what the stages behind the aggregate make of it before the one rounding to okind."""
    D, n = len(xs), np.asarray(xs[0]).size
    Q, order, ps, sel = agg.bulyan_round(part)
    check_q(Q, exact, n, what)
    rorder, rps, rsel = B.select(Q, f)
    assert order.tolist() == rorder.tolist(), (what, order, rorder)
    assert np.array_equal(bits64(ps), bits64(rps)), (what, ps, rps)
    assert sel.tolist() == rsel.tolist(), what
    a = B.aggregate(xs, kind, sel, f)
    B.assert_bits(out, B.round_out(a if a_of is None else a_of(a), okind), what + " output")
    if honest_only:
        assert sel.sum() == D - 2 * f and not sel[byzantine(D, f)].any(), (what, sel)
    return Q, order, sel, a


def submit_all(agg, part, xs):
    for k, x in enumerate(xs):
        agg.submit(part, k, x, 1.0)


# ------------------------------------------------------------------ the four assertions over D, f, sizes, dtypes

@pytest.mark.parametrize("kind,okind", PAIRS)
@pytest.mark.parametrize("D,f", DF)
def test_bulyan_rounds(fa, torch_gpu, D, f, kind, okind):
    with fa.Aggregator(1) as agg:
        for part, n in enumerate(NS, start=1):
            xs, exact = case(D, f, kind, n)
            agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, okind), D, mode=fa.TRIMMED)
            agg.set_bulyan(f, part)
            submit_all(agg, part, xs)
            out = agg.finalize(part)
            check_round(agg, part, out, xs, exact, kind, okind, f, "%s -> %s D %d f %d n %d" % (kind, okind, D, f, n))


@pytest.mark.parametrize("poison", ["nan", "inf"])
def test_a_byzantine_bucket_of_nan_or_inf(fa, torch_gpu, poison):
    D, f, n = 11, 2, 4099
    xs = [x.copy() for x in case(D, f, "f32", n)[0]]
    xs[1][:] = {"nan": np.nan, "inf": np.inf}[poison]  # the first Byzantine owner; the second stays far off
    exact = K.distances(xs, "f32")
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        agg.set_bulyan(f, 1)
        submit_all(agg, 1, xs)
        out = agg.finalize(1)
        Q, _, _, _ = check_round(agg, 1, out, xs, exact, "f32", "f32", f, poison)
        row = np.delete(Q[1], 1)
        assert (np.isnan(row) if poison == "nan" else row == np.inf).all() and np.isfinite(out).all()


# ------------------------------------------------------------------ composition

def test_the_aggregate_feeds_the_server_optimizer(fa, torch_gpu):
    D, f, n, kind = 7, 1, 4099, "bf16"
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.BF16, fa.BF16, D, mode=fa.TRIMMED)
        agg.set_server_opt(S.ADAM, part_id=1, **hp)
        agg.set_bulyan(f, 1)
        x0 = np.random.default_rng(SEED + 9).uniform(-1, 1, n).astype(F32)
        agg.set_server_opt_state(1, x=x0)
        ref = (x0, np.zeros(n, F32), np.zeros(n, F32))
        for step in (1, 2):
            xs = make_clients(n, D, f, kind, SEED + 40 + step)
            submit_all(agg, 1, xs)
            out = agg.finalize(1)
            Q, order, ps, sel = agg.bulyan_round(1)
            check_q(Q, K.distances(xs, kind), n, "step %d" % step)
            assert sel.sum() == D - 2 * f and not sel[byzantine(D, f)].any()
            ref = S.step(S.ADAM, B.aggregate(xs, kind, sel, f), *ref, **hp)
            x, m, v, k = agg.server_opt_state(1)
            assert k == step
            for got, exp, name in ((x, ref[0], "x"), (m, ref[1], "m"), (v, ref[2], "v")):
                B.assert_bits(got, exp, "step %d %s" % (step, name))
            B.assert_bits(out, S.round_out(ref[0], kind), "step %d output" % step)


@pytest.mark.parametrize("kind,okind", [("f32", "f32"), ("f32", "f16")])
def test_the_aggregate_feeds_the_noise_stage(fa, torch_gpu, kind, okind):
    D, f, n, stddev, part = 8, 1, 4099, 0.25, 3
    xs, exact = case(D, f, kind, n)
    with fa.Aggregator(1) as agg:
        agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, okind), D, mode=fa.TRIMMED)
        agg.set_bulyan(f, part)
        agg.set_noise(stddev, SEED, part)
        for rnd in (0, 1):
            submit_all(agg, part, xs)
            out = agg.finalize(part)
            check_round(agg, part, out, xs, exact, kind, okind, f, "noise round %d" % rnd,
                        a_of=lambda a: N.noisy(a, stddev, SEED, part, rnd))


@pytest.mark.parametrize("okind", ["bf16", "f16"])
def test_a_16_bit_output_is_rounded_once(fa, torch_gpu, okind):
    D, f, n = 7, 1, 4099
    xs, exact = case(D, f, "f32", n)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa_dt(fa, okind), D, mode=fa.TRIMMED)
        agg.set_bulyan(f, 1)
        submit_all(agg, 1, xs)
        check_round(agg, 1, agg.finalize(1), xs, exact, "f32", okind, f, "f32 -> " + okind)


# ------------------------------------------------------------------ layouts and calls

def one_gpu_round(fa, xs, kind, f):
    D, n = len(xs), np.asarray(xs[0]).size
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D, mode=fa.TRIMMED)
        agg.set_bulyan(f, 1)
        submit_all(agg, 1, xs)
        out = agg.finalize(1)
        return out, agg.bulyan_round(1)


def test_two_range_shards_match_one_gpu(fa, torch_gpu):
    D, f, n = 7, 1, 100003
    xs = make_clients(n, D, f, "f32", SEED + 6)
    exact = K.distances(xs, "f32")
    ref_out, (_, ref_order, _, _) = one_gpu_round(fa, xs, "f32", f)
    with fa.Aggregator(devices=[0, 0], shared_device=True) as agg:
        agg.set_bulyan(f)  # the context default: trimmed parts defined later take it
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        agg.define(2, n, fa.F32, fa.F32, D)  # a FedAvg part does not
        with pytest.raises(fa.FaError) as e:
            agg.bulyan_round(2)
        assert e.value.code == fa.ERR_STATE
        for how in ("finalize", "reduce", "reduce_parts"):
            submit_all(agg, 1, xs)
            if how == "finalize":
                out = agg.finalize(1)
            elif how == "reduce":
                agg.reduce(1)
                out = agg.copy_output(1)
            else:
                agg.reduce_parts([1])
                out = agg.finalize(1)  # only copies out
            _, order, _, _ = check_round(agg, 1, out, xs, exact, "f32", "f32", f, "two shards by " + how)
            assert order.tolist() == ref_order.tolist()
            B.assert_bits(out, ref_out, "two shards == one GPU, by " + how)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_range_pieces_match_one_piece(fa, torch_gpu, kind):
    D, f, n = 7, 1, 100003
    xs = make_clients(n, D, f, kind, SEED + 7)
    exact = K.distances(xs, kind)
    ref_out, (_, ref_order, _, _) = one_gpu_round(fa, xs, kind, f)
    with fa.Aggregator(1) as agg:
        agg.set_tuning(piece_span_kib=512, piece_split_kib=-1)
        agg.set_bulyan(f)
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D, mode=fa.TRIMMED)
        assert len(agg.pieces(1, 0, 0)) >= 2
        submit_all(agg, 1, xs)
        out = agg.finalize(1)
        _, order, _, _ = check_round(agg, 1, out, xs, exact, kind, kind, f, "pieces")
        assert order.tolist() == ref_order.tolist()
        B.assert_bits(out, ref_out, "pieces == one piece")


def test_reduce_part_twice_and_every_client_is_needed(fa, torch_gpu):
    D, f, n = 7, 1, 4099
    xs, exact = case(D, f, "f32", n)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        agg.set_bulyan(f, 1)
        with pytest.raises(fa.FaError) as e:
            agg.bulyan_round(1)  # never reduced with the stage
        assert e.value.code == fa.ERR_STATE
        agg.submit(1, 0, xs[0], 1.0)
        with pytest.raises(fa.FaError) as e:
            agg.reduce(1)
        assert e.value.code == fa.ERR_STATE
        submit_all(agg, 1, xs)
        agg.reduce(1)
        first = agg.copy_output(1)
        Q1 = agg.bulyan_round(1)[0]
        agg.reduce(1)  # the stage keeps no state: the same round again
        second = agg.copy_output(1)
        check_round(agg, 1, second, xs, exact, "f32", "f32", f, "second reducing call")
        B.assert_bits(second, first, "fa_reduce_part twice")
        assert np.array_equal(bits64(agg.bulyan_round(1)[0]), bits64(Q1)), "the same layout gave other bits"
        B.assert_bits(agg.finalize(1), first, "the finalize only copies out")


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_removing_the_stage_returns_to_the_trimmed_mean(fa, torch_gpu, kind):
    D, f, n = 8, 1, 4099
    xs, exact = case(D, f, kind, n)
    wide = [B.widen(x, kind) for x in xs]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D, mode=fa.TRIMMED, trim=2)
        submit_all(agg, 1, xs)
        plain = agg.finalize(1)
        B.assert_bits(plain, B.round_out(T.trimmed_f32(wide, 2), kind), "before the stage")
        agg.set_bulyan(f, 1)
        submit_all(agg, 1, xs)
        check_round(agg, 1, agg.finalize(1), xs, exact, kind, kind, f, "with the stage")
        agg.set_bulyan(None, 1)
        submit_all(agg, 1, xs)
        B.assert_bits(agg.finalize(1), plain, "stage removed: the trim is back")
        with pytest.raises(fa.FaError) as e:
            agg.bulyan_round(1)
        assert e.value.code == fa.ERR_STATE


def test_refusals(fa, torch_gpu):
    D, n = 7, 67
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.set_bulyan(1)
        assert e.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(e.value)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)
        agg.define(2, n, fa.F32, fa.F32, D)
        for part, name in ((1, "FA_LITERAL"), (2, "FA_FEDAVG")):
            with pytest.raises(fa.FaError) as e:
                agg.set_bulyan(1, part)
            assert e.value.code == fa.ERR_ARG and name in str(e.value)
        agg.define(3, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        for f, says in ((2, "f = 2"), (-2, "f = -2")):
            with pytest.raises(fa.FaError) as e:
                agg.set_bulyan(f, 3)
            assert e.value.code == fa.ERR_ARG and says in str(e.value)
        agg.set_bulyan(1)  # the context default
        with pytest.raises(fa.FaError) as e:  # checked against D at define time
            agg.define(4, n, fa.F32, fa.F32, 6, mode=fa.TRIMMED)
        assert e.value.code == fa.ERR_ARG and "f = 1" in str(e.value)
        agg.define(4, n, fa.F32, fa.F32, 6)  # FedAvg parts do not take it
        agg.define(5, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        xs, exact = case(D, 1, "f32", n)
        submit_all(agg, 5, xs)
        assert agg.host_read_kept(5) == 0
        check_round(agg, 5, agg.finalize(5), xs, exact, "f32", "f32", 1, "context default")
