"""GPU: MX8 receipts through a context (fa_set_mx8, fa_submit_mx8, fa_mx8_set_reference).

Round 1 from full receipts; round 2 from three MX8 receipts against round 1's output and two full ones: the result
must be the oracle's aggregate over the expanded values (tests/mx8_ref.py), bit for bit -- on one GPU, on range
shards, on range pieces, for FA_TRIMMED, under the clip stage and a server optimizer, and for 16-bit parts.  Then the
reference set by hand, the refusals, and what the part's other entries say while it takes MX8 receipts.
"""
import numpy as np
import pytest

import clip_ref as R
import mx8_ref as M
import server_opt_ref as S
import trimmed_ref as T

pytestmark = pytest.mark.gpu

F32, I8, U8 = np.float32, np.int8, np.uint8
N, D = 100003, 5
MX8_SLOTS = (0, 2, 4)  # round 2: these owners send MX8, the others full receipts


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def make_clients(n, D, kind, seed):
    rng = np.random.default_rng(seed)
    return [R.round_out(rng.uniform(-1, 1, n).astype(F32), kind) for _ in range(D)]


def plain_aggregate(O, xs, kind, w):
    if kind == "bf16":
        return O.fedavg([np.ascontiguousarray(x) for x in xs], w, out_dtype="f32")
    return O.fedavg([R.widen(x, kind) for x in xs], w)


def owner_update(g, okind, n, seed):
    """What an owner does: delta = fl32(x - g) against the reply g it last loaded, then the encoder."""
    rng = np.random.default_rng(seed)
    gw = R.widen(g, okind)
    x = (gw + F32(0.05) * rng.standard_normal(n).astype(F32)).astype(F32)
    return M.encode((x - gw).astype(F32))


def second_round(fa, agg, part, g, kind, okind, w, seed, n=N):
    """Submits round 2 (MX8 from MX8_SLOTS, one of them from pinned memory; full from the rest); returns the values
    the slots must hold."""
    full = make_clients(n, D, kind, seed)
    xs, keep = [], []
    for k in range(D):
        if k not in MX8_SLOTS:
            agg.submit(part, k, full[k], w[k])
            xs.append(full[k])
            continue
        q, e = owner_update(g, okind, n, seed + 100 + k)
        if k == 2:
            pq, pe = pinned_copy(fa, q), pinned_copy(fa, e)
            keep += [pq, pe]
            agg.submit_mx8(part, k, pq.view(I8), pe.view(U8), w[k], pinned=True)
        else:
            agg.submit_mx8(part, k, q, e, w[k])
            q[:] = 0  # reusable on return: the library took its copy
        xs.append(M.expand(*owner_update(g, okind, n, seed + 100 + k), 0, kind, g, okind))
    return xs, keep


def pinned_copy(fa, host):
    p = fa.PinnedBuffer(host.nbytes)
    p.view(host.dtype)[:] = host
    return p


LAYOUTS = {
    "one GPU": lambda fa: fa.Aggregator(1),
    "two shards": lambda fa: fa.Aggregator(devices=[0, 0], shared_device=True),
    "three shards": lambda fa: fa.Aggregator(devices=[0, 0, 0], shared_device=True),
    "pieces": lambda fa: fa.Aggregator(1),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind,okind", [("f32", "f32"), ("bf16", "bf16"), ("f32", "f16")])
def test_fedavg_two_rounds(fa, O, torch_gpu, kind, okind, layout):
    part, w = 3, O.weights(D)
    with LAYOUTS[layout](fa) as agg:
        if layout == "pieces":
            agg.set_tuning(piece_span_kib=64, piece_split_kib=-1)
        agg.set_mx8()  # the context default
        agg.define(part, N, fa_dt(fa, kind), fa_dt(fa, okind), D)
        if layout == "pieces":
            assert len(agg.pieces(part, 0, 0)) >= 3
        xs1 = make_clients(N, D, kind, 1)
        for k in range(D):
            agg.submit(part, k, xs1[k], w[k])
        g = agg.finalize(part)
        R.assert_bits(g, R.round_out(plain_aggregate(O, xs1, kind, w), okind), "round 1")
        xs2, keep = second_round(fa, agg, part, g, kind, okind, w, 2)
        assert agg.progress(part) == (D, 0)
        out = agg.finalize(part)
        R.assert_bits(out, R.round_out(plain_aggregate(O, xs2, kind, w), okind), "round 2, %s" % layout)
        del keep


def test_trimmed_part(fa, O, torch_gpu):
    part, w = 1, O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(part, N, fa.F32, fa.F32, D, mode=fa.TRIMMED, trim=1)
        agg.set_mx8(True, part)
        xs1 = make_clients(N, D, "f32", 11)
        for k in range(D):
            agg.submit(part, k, xs1[k], w[k])
        g = agg.finalize(part)
        R.assert_bits(g, T.trimmed_f32(xs1, 1), "round 1")
        xs2, keep = second_round(fa, agg, part, g, "f32", "f32", w, 12)
        R.assert_bits(agg.finalize(part), T.trimmed_f32(xs2, 1), "round 2")
        del keep


def test_clip_stage_measures_the_expanded_values(fa, O, torch_gpu):
    part, w, C = 2, O.weights(D), 50.0  # between the MX8 owners' norms (0.05 sqrt(N) = 16) and the full ones' (~260)
    with fa.Aggregator(1) as agg:
        agg.define(part, N, fa.F32, fa.F32, D)
        agg.set_clip(C, part)
        agg.set_mx8(True, part)
        xs1 = make_clients(N, D, "f32", 21)
        for k in range(D):
            agg.submit(part, k, xs1[k], w[k])
        g = agg.finalize(part)  # the bootstrap round: the plain aggregate, the reference of both stages
        R.assert_bits(g, plain_aggregate(O, xs1, "f32", w), "round 1")
        xs2, keep = second_round(fa, agg, part, g, "f32", "f32", w, 22)
        out = agg.finalize(part)
        Q, scales, included, n_clipped = agg.clip_round(part)
        for k in range(D):
            exact = R.sumsq(xs2[k], g)
            assert abs(Q[k] - exact) <= R.sumsq_bound(N, exact), (k, Q[k], exact)
        assert 0 < n_clipped < D  # the MX8 owners moved 0.05 per element, the full ones a fresh uniform draw
        R.assert_bits(out, R.aggregate(O, xs2, "f32", w, scales, included, g), "round 2")
        del keep


@pytest.mark.parametrize("okind", ["f32", "bf16"])
def test_server_optimizer_reference_is_the_stepped_output(fa, O, torch_gpu, okind):
    part, w = 4, O.weights(D)
    hp = dict(lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3)
    with fa.Aggregator(1) as agg:
        agg.set_server_opt(S.ADAM, **hp)
        agg.set_mx8()
        agg.define(part, N, fa.F32, fa_dt(fa, okind), D)
        x0 = np.random.default_rng(31).uniform(-1, 1, N).astype(F32)
        agg.set_server_opt_state(part, x=x0)
        state = (x0, np.zeros(N, F32), np.zeros(N, F32))
        xs1 = make_clients(N, D, "f32", 32)
        for k in range(D):
            agg.submit(part, k, xs1[k], w[k])
        g = agg.finalize(part)
        state = S.step(S.ADAM, plain_aggregate(O, xs1, "f32", w), *state, **hp)
        R.assert_bits(g, S.round_out(state[0], okind), "round 1: the stepped model")
        xs2, keep = second_round(fa, agg, part, g, "f32", okind, w, 33)  # against g, not against the aggregate
        out = agg.finalize(part)
        state = S.step(S.ADAM, plain_aggregate(O, xs2, "f32", w), *state, **hp)
        R.assert_bits(out, S.round_out(state[0], okind), "round 2")
        del keep


def test_set_reference_then_relative_and_absolute_submits(fa, O, torch_gpu):
    part, n, w = 5, 4099, O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(part, n, fa.F32, fa.F32, D)
        agg.set_mx8(True, part)
        q, e = M.encode(np.random.default_rng(41).standard_normal(n).astype(F32))
        with pytest.raises(fa.FaError) as ei:  # never reduced, no reference
            agg.submit_mx8(part, 0, q, e, w[0])
        assert ei.value.code == fa.ERR_STATE and "part %d" % part in str(ei.value) and "reference" in str(ei.value)
        assert agg.progress(part) == (0, 0)
        agg.submit_mx8(part, 0, q, e, w[0], absolute=True)  # absolute mode needs none
        g = np.random.default_rng(42).uniform(-1, 1, n).astype(F32)
        agg.set_mx8_reference(part, g)
        R.assert_bits(agg.copy_output(part), g, "the reference, as a round's output")
        xs = [M.expand(q, e, 0, "f32")]
        for k in range(1, D):
            qk, ek = owner_update(g, "f32", n, 50 + k)
            agg.submit_mx8(part, k, qk, ek, w[k])
            xs.append(M.expand(qk, ek, 0, "f32", g, "f32"))
        assert agg.host_read_kept(part) == 0
        R.assert_bits(agg.finalize(part), plain_aggregate(O, xs, "f32", w), "all five compressed")


def test_mx8_overwrites_a_full_receipt_and_the_reverse(fa, O, torch_gpu):
    part, n, w = 6, 4099, O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(part, n, fa.F32, fa.F32, D)
        agg.set_mx8(True, part)
        g = np.random.default_rng(61).uniform(-1, 1, n).astype(F32)
        agg.set_mx8_reference(part, g)
        xs = make_clients(n, D, "f32", 62)
        for k in range(D):
            agg.submit(part, k, xs[k], w[k])
        q, e = owner_update(g, "f32", n, 63)
        agg.submit_mx8(part, 1, q, e, 0.25)  # full, then MX8: the slot holds the MX8 values and weight
        q3, e3 = owner_update(g, "f32", n, 64)
        agg.submit_mx8(part, 3, q3, e3, w[3])
        agg.submit(part, 3, xs[3], w[3])       # MX8, then full: the full ones
        assert agg.progress(part) == (D, 0)
        xs[1] = M.expand(q, e, 0, "f32", g, "f32")
        w2 = np.array(w, F32)
        w2[1] = 0.25
        R.assert_bits(agg.finalize(part), plain_aggregate(O, xs, "f32", w2), "overwritten")


def test_small_pinned_receipts_are_not_kept_host_side_and_eager_is_off(fa, O, torch_gpu):
    part, n, w = 7, 257, O.weights(D)
    xs = make_clients(n, D, "f32", 71)
    with fa.Aggregator(1, eager=True) as agg:
        agg.set_mx8()
        agg.define(part, n, fa.F32, fa.F32, D)
        agg.define(part + 1, n, fa.F32, fa.F32, D)
        pins = []
        for k in range(D):
            pins.append(pinned_copy(fa, xs[k]))
            agg.submit(part, k, pins[k].view(F32), w[k], pinned=True)
            agg.submit(part + 1, k, xs[k], w[k])
            assert agg.progress(part) == (k + 1, 0)  # non-eager
        assert agg.host_read_kept(part) == 0
        agg.reduce_parts([part, part + 1])  # batched: the output still becomes the reference
        g = agg.finalize(part)
        R.assert_bits(g, plain_aggregate(O, xs, "f32", w), "round 1")
        R.assert_bits(agg.finalize(part + 1), g, "round 1, the other part of the batch")
        xs2, keep = second_round(fa, agg, part, g, "f32", "f32", w, 72, n=n)
        R.assert_bits(agg.finalize(part), plain_aggregate(O, xs2, "f32", w), "round 2")
        # switched off: a relative submit is refused, full rounds go on
        agg.set_mx8(False, part)
        with pytest.raises(fa.FaError) as ei:
            agg.submit_mx8(part, 0, *owner_update(g, "f32", n, 73), w[0])
        assert ei.value.code == fa.ERR_STATE and "fa_set_mx8" in str(ei.value)
        for k in range(D):
            agg.submit(part, k, xs[k], w[k])
        R.assert_bits(agg.finalize(part), g, "after fa_set_mx8(0)")
        # on again: the output of a round reduced with it off is no reference
        agg.set_mx8(True, part)
        with pytest.raises(fa.FaError) as ei:
            agg.submit_mx8(part, 0, *owner_update(g, "f32", n, 73), w[0])
        assert ei.value.code == fa.ERR_STATE and "reference" in str(ei.value)
        del keep, pins


def test_refusals(fa, O, torch_gpu):
    n = 67
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as ei:
            agg.set_mx8()
        assert ei.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(ei.value)
        agg.set_mx8(False)  # switching nothing off is fine
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)
        with pytest.raises(fa.FaError) as ei:
            agg.set_mx8(True, 1)
        assert ei.value.code == fa.ERR_ARG and "FA_LITERAL" in str(ei.value)
        agg.set_mx8()
        agg.define(2, n, fa.F32, fa.F32, D, mode=fa.LITERAL)  # ignores the context default
        q, e = M.encode(np.ones(n, F32))
        with pytest.raises(fa.FaError) as ei:
            agg.submit_mx8(2, 0, q, e, absolute=True)
        assert ei.value.code == fa.ERR_STATE
        agg.define(3, n, fa.F32, fa.F32, D)
        with pytest.raises(fa.FaError) as ei:
            agg.submit_mx8(3, D, q, e, absolute=True)
        assert ei.value.code == fa.ERR_ARG and "slot" in str(ei.value)
        with pytest.raises(fa.FaError) as ei:
            fa.check(fa.lib().fa_submit_mx8(agg.handle, 3, 0, q.ctypes.data, e.ctypes.data, 1.0, 0x10))
        assert ei.value.code == fa.ERR_ARG and "flags" in str(ei.value)
        with pytest.raises(fa.FaError) as ei:
            fa.check(fa.lib().fa_submit_mx8(agg.handle, 3, 0, None, e.ctypes.data, 1.0, fa.MX8_ABSOLUTE))
        assert ei.value.code == fa.ERR_ARG and "q is null" in str(ei.value)
