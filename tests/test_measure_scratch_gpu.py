"""GPU: the clip stage's norm pass and the Krum stage's distance pass share one scratch per GPU of a context
(MeasureScratch in csrc/fa_host.h).  One context holds a clip part (D = 8) and two Krum parts (D = 33, f = 10 and
D = 5, f = 1), reduced together round after round, so the scratch grows from the clip stage's layout (8 sums) to a
Krum one (33 x 33 matrix, 528 pairs of partials) and then serves a smaller one (5 x 5), and the raw entries run
on it afterwards.  Every output and every report must be bit-equal to the same part alone on a context of its
own with the same layout and inputs, where nothing else ever touched the scratch.

The inputs are those of test_clip_gpu.py (even clients pass C = 0.05 sqrt(n), odd ones are clipped, by a factor
of 5 at least either way) and test_krum_gpu.py (the honest set is selected, by a factor of 600 in the scores), so
the expected flags do not hang on the summation order; the alone runs assert them.
"""
import numpy as np
import pytest

import clip_ref as R
import test_clip_gpu as CG
import test_krum_gpu as KG

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x5C7A
ROUNDS = 3
N = 4099
CLIP_D = 8
KRUM = {2: (33, 10), 3: (5, 1)}  # part: (D, f)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_report(got, want, what):
    """Two clip_round or krum_round tuples, bit for bit."""
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i)
        assert a.tobytes() == b.tobytes(), "%s: field %d differs: %r != %r" % (what, i, a, b)


def krum_inputs(part, n, r):
    D, f = KRUM[part]
    return KG.make_clients(n, D, f, "f32", SEED + 100 * part + r)


def define(fa, agg, part, n):
    if part == 1:
        agg.define(1, n, fa.F32, fa.F32, CLIP_D)
        agg.set_clip(CG.bound_c(n), 1)
    else:
        D, f = KRUM[part]
        agg.define(part, n, fa.F32, fa.F32, D)
        agg.set_krum(f, None, part)


def report(agg, part):
    return agg.clip_round(part) if part == 1 else agg.krum_round(part)


def alone(fa, O, layout, part, n):
    """The part's ROUNDS rounds on a context of its own: per round (inputs, output, report)."""
    D = CLIP_D if part == 1 else KRUM[part][0]
    w = O.weights(D)
    rounds = []
    with fa.Aggregator(**layout) as agg:
        define(fa, agg, part, n)
        g = None
        for r in range(ROUNDS):
            if part == 1:  # round r's receipts surround the model the round before sent out
                xs = CG.make_clients(CG.make_ref(n, SEED) if g is None else g, CLIP_D, "f32", SEED + r)
            else:
                xs = krum_inputs(part, n, r)
            CG.submit_all(agg, part, xs, w)
            agg.reduce_parts([part])
            out = agg.finalize(part)
            rep = report(agg, part)
            if part == 1:
                Q, scales, included, n_clipped = rep
                if g is None:  # the bootstrap
                    assert not Q.any() and (scales == 1).all() and included.all() and n_clipped == 0
                else:
                    assert included.all() and (scales[0::2] == 1).all() and (scales[1::2] < 1).all() and n_clipped == 4
                    CG.check_q(Q, xs, "f32", g, "alone round %d" % (r + 1))
                g = out.copy()
            else:
                assert rep[2].tolist() == KG.honest_flags(*KRUM[part]).tolist()
            rounds.append((xs, out, rep))
    return rounds


@pytest.mark.parametrize("layout,n3", [(dict(n_gpus=1), N), (dict(devices=[0, 0], shared_device=True), 100003)],
                         ids=["one gpu", "two shards"])
def test_clip_and_krum_parts_share_a_context(fa, O, torch_gpu, layout, n3):
    ns = {1: N, 2: N, 3: n3}
    ref = {part: alone(fa, O, layout, part, ns[part]) for part in (1, 2, 3)}
    with fa.Aggregator(**layout) as agg:
        for part in (1, 2, 3):
            define(fa, agg, part, ns[part])
        for r in range(ROUNDS):
            for part in (1, 2, 3):
                xs = ref[part][r][0]
                CG.submit_all(agg, part, xs, O.weights(len(xs)))
            agg.reduce_parts([1, 2, 3])
            for part in (1, 2, 3):
                what = "round %d part %d" % (r + 1, part)
                R.assert_bits(agg.finalize(part), ref[part][r][1], what + " output")
                same_report(report(agg, part), ref[part][r][2], what + " report")
        # the raw entries on the same context (its scratch) against the context-less calls (scratch of their own)
        xs, _, _ = ref[1][ROUNDS - 1]
        g = ref[1][ROUNDS - 2][1]
        devs = [CG.dev_buf(torch_gpu, x, "f32", 0) for x in xs]
        dg = CG.dev_buf(torch_gpu, g, "f32", 0)
        q_ctx, q_own = fa.clip_sumsq_device(devs, N, fa.F32, dg, ctx=agg), fa.clip_sumsq_device(devs, N, fa.F32, dg)
        assert np.array_equal(bits64(q_ctx), bits64(q_own)), (q_ctx, q_own)
        CG.check_q(q_ctx, xs, "f32", g, "raw norm pass on the context")
        xs = ref[2][ROUNDS - 1][0]
        devs = [CG.dev_buf(torch_gpu, x, "f32", 0) for x in xs]
        d_ctx, d_own = fa.pairdist_device(devs, N, fa.F32, ctx=agg), fa.pairdist_device(devs, N, fa.F32)
        assert np.array_equal(bits64(d_ctx), bits64(d_own))
        KG.check_q(d_ctx, xs, "f32", "raw distance pass on the context")
