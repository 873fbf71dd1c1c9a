"""GPU: the geomed stage through a context (fa_set_geomed, fa.h "Geomed stage") against tests/geomed_ref.py.

A round's sums may be added in any order, so one pass may differ from the exact one in its last bits and the next
pass's weights with it: a round is checked by its trace (geomed_ref.check_trace).  For every reported pass t, Q^t is
within n * 2^-53 * exact of the exactly rounded sum against v^t rebuilt from the reported alpha^t; alpha^{t+1}, the
flags and the objective are bit-equal to rules 3-4 applied to the reported Q^t; and the output is bit-equal to the
chain under the last row of weights.  On top of that the data are built so that the rule has to do its job: the
owners far away end with a small share of the mass.
"""
import numpy as np
import pytest

import geomed_ref as G
import noise_ref as N
import server_opt_ref as S

pytestmark = pytest.mark.gpu

F16, F32, F64, U16 = np.float16, np.float32, np.float64, np.uint16
SEED = 0x6E0A
NU = 1e-6


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def make_clients(n, D, bad, kind, seed):
    """Honest owners g + 0.1 u; the first `bad` owners at g + 100."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, n).astype(F32)
    xs = []
    for k in range(D):
        x = g + F32(100.0) if k < bad else g + F32(0.1) * rng.uniform(-1, 1, n).astype(F32)
        xs.append(G.round_out(x.astype(F32), kind))
    return xs


def submit_all(agg, part, xs, w):
    for k, x in enumerate(xs):
        agg.submit(part, k, x, w[k])


def round_and_check(agg, O, part, xs, kind, okind, w, T, what, how="finalize"):
    submit_all(agg, part, xs, w)
    if how == "finalize":
        out = agg.finalize(part)
    elif how == "reduce":
        agg.reduce(part)
        out = agg.copy_output(part)
    else:
        agg.reduce_parts([part])
        out = agg.finalize(part)  # only copies out
    trace = agg.geomed_round(part)
    a = G.check_trace(O, xs, kind, w, NU, trace, what)
    G.assert_bits(out, G.round_out(a, okind), what + ": output")
    return out, trace, a


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("D,bad,T", [(1, 0, 2), (3, 1, 1), (8, 2, 4), (11, 3, 8), (33, 10, 3), (65, 20, 2), (128, 40, 2)])
def test_rounds_by_trace(fa, O, torch_gpu, D, bad, T, kind):
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        for part, n in enumerate((67, 4099, 100003) if D <= 33 else (4099,), start=1):
            xs = make_clients(n, D, bad, kind, SEED + n + D)
            agg.define(part, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
            agg.set_geomed(T, NU, part)
            assert agg.geomed(part) == (T, float(F32(NU)))
            what = "%s D %d T %d n %d" % (kind, D, T, n)
            out, (q, wr, inc, obj), a = round_and_check(agg, O, part, xs, kind, kind, w, T, what)
            assert q.shape == (T, D) and inc.all()
            # The owners at g + 100 lose their mass.  With s_t their share of the weights at pass t, v^t lies s_t of
            # the way to them (the honest spread of 0.1 is nothing against 100), so beta_bad / beta_honest =
            # s_t / (1 - s_t) and s_{t+1} = s_0 r / (s_0 r + 1 - s_0) with r = s_t / (1 - s_t).  From s_0 <= 0.35 three
            # passes give s_3 <= 0.077 < s_0 / 4.  Every pass lowers the objective (Weiszfeld).
            s0 = float(w[:bad].sum() / w.sum())
            if bad and T >= 3 and s0 <= 0.35:
                assert wr[-1][:bad].sum() < 0.25 * w[:bad].sum(), (what, wr[-1])
                assert all(obj[t + 1] <= obj[t] for t in range(T - 1)), (what, obj)


def test_a_nan_bucket_and_a_zero_weight(fa, O, torch_gpu):
    n, D, T = 4099, 6, 3
    xs = make_clients(n, D, 1, "f32", SEED + 1)
    xs[2][n - 1] = np.nan
    w = O.weights(D).copy()
    w[4] = 0.0
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_geomed(T, NU, 1)
        out, (q, wr, inc, obj), _ = round_and_check(agg, O, 1, xs, "f32", "f32", w, T, "nan bucket")
        assert inc.tolist() == [True, True, False, True, False, True] and np.isfinite(out).all()
        assert q.shape == (T, D) and (q[:, [2, 4]] == 0).all() and (wr[:, [2, 4]] == 0).all()  # the void pass is not reported
        ref = G.geomed_round(O, xs, "f32", w, T, NU)
        assert ref["voided"] == 1 and ref["included"].tolist() == inc.tolist()
        G.assert_bits(wr[0], ref["weights"][0], "alpha^0 after the void pass comes from w")
        # an inf is a non-finite bucket too; 3e38 against the others is an overflow of d: excluded by rule 3, no repeat
        xs = make_clients(n, D, 0, "f32", SEED + 2)
        xs[0][5] = -np.inf
        xs[3][7] = 3e38
        for k in (1, 2, 4, 5):
            xs[k][7] = -3e38  # v[7] = 3e38 (1 - 4) / 6 = -1.5e38 once owner 0 is out: owner 3 is 4.5e38 away
        w = np.full(D, 1.0 / D, F32)
        out, (q, wr, inc, obj), _ = round_and_check(agg, O, 1, xs, "f32", "f32", w, T, "inf bucket and overflow")
        assert inc.tolist() == [False, True, True, False, True, True] and np.isfinite(out).all()
        assert q[0, 3] == np.inf and (q[1:, 3] == 0).all()


def test_everyone_excluded_gives_zero(fa, O, torch_gpu):
    n, D = 4099, 4
    xs = make_clients(n, D, 0, "f32", SEED + 3)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_geomed(2, NU, 1)
        out, (q, wr, inc, obj), _ = round_and_check(agg, O, 1, xs, "f32", "f32", np.zeros(D, F32), 2, "all weights 0")
        assert not inc.any() and q.shape == (0, D) and wr.shape == (1, D) and out.view(np.uint32).tolist() == [0] * n
        for x in xs:
            x[7] = np.nan
        out, (q, wr, inc, obj), _ = round_and_check(agg, O, 1, xs, "f32", "f32", O.weights(D), 2, "all buckets NaN")
        assert not inc.any() and q.shape == (0, D) and out.view(np.uint32).tolist() == [0] * n


def one_gpu_round(fa, O, xs, kind, w, T):
    D, n = len(xs), np.asarray(xs[0]).size
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.set_geomed(T, NU, 1)
        out, trace, _ = round_and_check(agg, O, 1, xs, kind, kind, w, T, "one GPU")
        return out, trace


def same_weights(a, b):
    return a[1].shape == b[1].shape and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_two_range_shards(fa, O, torch_gpu):
    D, bad, n, T = 5, 1, 100003, 3
    xs = make_clients(n, D, bad, "f32", SEED + 6)
    w = O.weights(D)
    ref_out, ref_trace = one_gpu_round(fa, O, xs, "f32", w, T)
    with fa.Aggregator(devices=[0, 0], shared_device=True) as agg:
        agg.set_geomed(T, NU)  # the context default: FedAvg parts defined later take it
        agg.define(1, n, fa.F32, fa.F32, D)
        assert agg.geomed(1) == (T, float(F32(NU))) and agg.geomed() == (T, float(F32(NU)))
        for how in ("finalize", "reduce", "reduce_parts"):
            out, trace, _ = round_and_check(agg, O, 1, xs, "f32", "f32", w, T, "two shards by " + how, how)
            if same_weights(trace, ref_trace):
                G.assert_bits(out, ref_out, "two shards == one GPU, by " + how)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_range_pieces(fa, O, torch_gpu, kind):
    D, bad, n, T = 5, 1, 100003, 3
    xs = make_clients(n, D, bad, kind, SEED + 7)
    w = O.weights(D)
    ref_out, ref_trace = one_gpu_round(fa, O, xs, kind, w, T)
    with fa.Aggregator(1) as agg:
        agg.set_tuning(piece_span_kib=512, piece_split_kib=-1)
        agg.set_geomed(T, NU)
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        assert len(agg.pieces(1, 0, 0)) >= 2
        out, trace, _ = round_and_check(agg, O, 1, xs, kind, kind, w, T, "pieces")
        if same_weights(trace, ref_trace):
            G.assert_bits(out, ref_out, "pieces == one piece")


@pytest.mark.parametrize("kind,okind", [("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f32", "f16")])
def test_16_bit_in_and_out(fa, O, torch_gpu, kind, okind):
    D, bad, n, T = 9, 2, 4099, 3
    xs = make_clients(n, D, bad, kind, SEED + 8)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, okind), D)
        agg.set_geomed(T, NU, 1)
        round_and_check(agg, O, 1, xs, kind, okind, O.weights(D), T, "%s -> %s" % (kind, okind))


@pytest.mark.parametrize("order", ["opt first", "geomed first"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_the_aggregate_feeds_the_server_optimizer(fa, O, torch_gpu, kind, order):
    D, bad, n, T = 5, 1, 4099, 2
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        if order == "opt first":
            agg.set_server_opt(S.ADAM, part_id=1, **hp)
            agg.set_geomed(T, NU, 1)
        else:
            agg.set_geomed(T, NU, 1)
            agg.set_server_opt(S.ADAM, part_id=1, **hp)
        x0 = np.random.default_rng(SEED + 9).uniform(-1, 1, n).astype(F32)
        agg.set_server_opt_state(1, x=x0)
        ref = (x0, np.zeros(n, F32), np.zeros(n, F32))
        for step in (1, 2):
            xs = make_clients(n, D, bad, kind, SEED + 40 + step)
            submit_all(agg, 1, xs, w)
            out = agg.finalize(1)
            a = G.check_trace(O, xs, kind, w, NU, agg.geomed_round(1), "step %d" % step)
            ref = S.step(S.ADAM, a, *ref, **hp)
            x, m, v, k = agg.server_opt_state(1)
            assert k == step
            for got, exp, name in ((x, ref[0], "x"), (m, ref[1], "m"), (v, ref[2], "v")):
                G.assert_bits(got, exp, "%s %s step %d %s" % (kind, order, step, name))
            G.assert_bits(out, S.round_out(ref[0], kind), "step %d output" % step)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_the_aggregate_feeds_the_noise_stage(fa, O, torch_gpu, kind):
    D, bad, n, T, stddev, seed = 5, 1, 4099, 2, 0.05, 0x5EEDFACE12345678
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.set_noise(stddev, seed, 1)
        agg.set_geomed(T, NU, 1)
        for rnd in range(2):
            xs = make_clients(n, D, bad, kind, SEED + 50 + rnd)
            submit_all(agg, 1, xs, w)
            out = agg.finalize(1)
            a = G.check_trace(O, xs, kind, w, NU, agg.geomed_round(1), "round %d" % rnd)
            G.assert_bits(out, G.round_out(N.noisy(a, stddev, seed, 1, rnd), kind), "noise round %d" % rnd)


def test_removed_stage_is_plain_fedavg_and_needs_every_client(fa, O, torch_gpu):
    D, n = 5, 4099
    xs = make_clients(n, D, 1, "f32", SEED + 10)
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_geomed(2, NU, 1)
        agg.submit(1, 0, xs[0], w[0])
        for call in (lambda: agg.reduce_parts([1, 2], weights=[w, w]), lambda: agg.reduce(1, weights=w),
                     lambda: agg.geomed_round(1)):  # every client needed; never reduced with the stage
            with pytest.raises(fa.FaError) as e:
                call()
            assert e.value.code == fa.ERR_STATE
        submit_all(agg, 2, xs, w)
        round_and_check(agg, O, 1, xs, "f32", "f32", w, 2, "a geomed part of a batch", "reduce_parts")
        G.assert_bits(agg.finalize(2), O.fedavg(xs, w), "the plain part")
        agg.set_geomed(0, part=1)
        assert agg.geomed(1) == (0, 0.0)
        submit_all(agg, 1, xs, w)
        G.assert_bits(agg.finalize(1), O.fedavg(xs, w), "stage removed")
        with pytest.raises(fa.FaError) as e:
            agg.geomed_round(1)
        assert e.value.code == fa.ERR_STATE


def test_refusals_and_an_eager_context(fa, O, torch_gpu):
    D, n = 5, 67
    w = O.weights(D)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.set_geomed(3)
        assert e.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(e.value)
    with fa.Aggregator(1, eager=True) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)
        agg.define(2, n, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        for part, name in ((1, "FA_LITERAL"), (2, "FA_TRIMMED")):
            with pytest.raises(fa.FaError) as e:
                agg.set_geomed(3, NU, part)
            assert e.value.code == fa.ERR_ARG and name in str(e.value)
        agg.define(3, n, fa.F32, fa.F32, D)
        for iters, nu, says in ((65, NU, "iters = 65"), (-1, NU, "iters = -1"), (3, 0.0, "nu"), (3, float("inf"), "nu")):
            with pytest.raises(fa.FaError) as e:
                agg.set_geomed(iters, nu, 3)
            assert e.value.code == fa.ERR_ARG and says in str(e.value)
        agg.set_geomed(3, NU, 3)
        for call, says in ((lambda: agg.set_clip(1.0, 3), "geomed"), (lambda: agg.set_krum(1, None, 3), "geomed")):
            with pytest.raises(fa.FaError) as e:
                call()
            assert e.value.code == fa.ERR_ARG and says in str(e.value)
        agg.define(4, n, fa.F32, fa.F32, D)
        agg.set_clip(1.0, 4)
        with pytest.raises(fa.FaError) as e:
            agg.set_geomed(3, NU, 4)
        assert e.value.code == fa.ERR_ARG and "clip" in str(e.value)
        agg.define(6, n, fa.F32, fa.F32, D)
        agg.set_krum(1, None, 6)
        with pytest.raises(fa.FaError) as e:
            agg.set_geomed(3, NU, 6)
        assert e.value.code == fa.ERR_ARG and "Krum" in str(e.value)
        agg.set_geomed(3, NU)  # the context default
        for call in (lambda: agg.set_clip(1.0), lambda: agg.set_krum(1)):
            with pytest.raises(fa.FaError) as e:
                call()
            assert e.value.code == fa.ERR_ARG and "geomed" in str(e.value)
        with pytest.raises(fa.FaError) as e:  # checked against D at define time
            agg.define(5, n, fa.F32, fa.F32, 129)
        assert e.value.code == fa.ERR_ARG and "at most 128" in str(e.value)
        agg.define(5, n, fa.F32, fa.F32, D)  # takes the context's stage: non-eager, never kept host-side
        xs = make_clients(n, D, 1, "f32", SEED + 11)
        pins = [fa.PinnedBuffer(n * 4) for _ in range(D)]
        for k in range(D):
            pins[k].view(F32)[:] = xs[k]
            agg.submit(5, k, pins[k].view(F32), w[k], pinned=True)
            assert agg.progress(5) == (k + 1, 0)
        assert agg.host_read_kept(5) == 0
        out = agg.finalize(5)
        a = G.check_trace(O, xs, "f32", w, NU, agg.geomed_round(5), "eager context")
        G.assert_bits(out, a, "eager context: output")
        agg.set_geomed(0)
        agg.set_clip(1.0)  # the default stage gone: the clip default is accepted again
