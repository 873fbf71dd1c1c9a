"""GPU: the sign-vote stage through Aggregator (fa_set_sign, fa_submit_sign, fa_copy_sign_planes) against
tests/sign_ref.py, every bit: a bootstrap round and two relative rounds on one GPU, two range shards and range pieces;
the planes rebuild the reply; noise and a server optimizer behind the stage; the refusals."""
import numpy as np
import pytest

import server_opt_ref as SO
import sign_ref as S

pytestmark = pytest.mark.gpu

F32 = np.float32
N, ETA = 20000 + 37, 0.01
LAYOUTS = {
    "one GPU": lambda fa: fa.Aggregator(1),
    "two shards": lambda fa: fa.Aggregator(devices=[0, 0], shared_device=True),
    "pieces": lambda fa: fa.Aggregator(1),
}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "bf16": fa.BF16, "f16": fa.F16}[kind]


def vote_round(agg, part, D, seed):
    """Submits D receipts; returns them."""
    bits = S.receipts(D, N, seed)
    for k in range(D):
        agg.submit_sign(part, k, bits[k])
    return bits


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("D,rule,margin,okind", [(5, S.MAJORITY, 1, "f32"), (8, S.MAJORITY, 2, "bf16"), (8, S.MEAN, 1, "f32"),
                                                (5, S.MEAN, 1, "f16")])
def test_three_rounds(fa, torch_gpu, D, rule, margin, okind, layout):
    part, planes = 3, rule == S.MAJORITY
    with LAYOUTS[layout](fa) as agg:
        if layout == "pieces":
            agg.set_tuning(piece_span_kib=64, piece_split_kib=-1)
        agg.define(part, N, fa.F32, fa_dt(fa, okind), D)
        if layout == "pieces":
            assert len(agg.pieces(part, 0, 0)) >= 2
        agg.set_sign(part, ETA, rule, margin, planes=planes)
        g = None  # the bootstrap round is absolute; then the reference is the previous output
        for rnd in range(3):
            bits = vote_round(agg, part, D, 10 * D + rnd)
            out = agg.finalize(part)
            gw = None if g is None else S.widen(g, okind)
            a, neg, pos = S.vote(bits, N, ETA, rule, margin, gw)
            S.assert_bits(out, S.round_out(a, okind), "round %d, %s" % (rnd, layout))
            if planes:  # an owner holding g and the planes rebuilds the reply
                gneg, gpos = agg.copy_sign_planes(part)
                assert np.array_equal(gneg, neg) and np.array_equal(gpos, pos), "planes, round %d" % rnd
                t = np.where(S.unpack(gneg, 0, N), -F32(ETA), np.where(S.unpack(gpos, 0, N), F32(ETA), F32(0))).astype(F32)
                S.assert_bits(out, S.round_out(t if gw is None else (gw + t).astype(F32), okind), "rebuilt reply")
            g = out


@pytest.mark.parametrize("okind", ["f32", "bf16"])
def test_noise_and_server_optimizer_follow(fa, torch_gpu, okind):
    D, hp, sd, seed = 5, dict(lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3), 0.25, 77
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa_dt(fa, okind), D)
        agg.set_sign(1, ETA, S.MAJORITY, 1)
        agg.set_noise(sd, seed, 1)
        agg.define(2, N, fa.F32, fa_dt(fa, okind), D)
        agg.set_server_opt(SO.ADAM, part_id=2, **hp)
        agg.set_sign(2, ETA, S.MEAN)
        g1 = g2 = state = None
        for rnd in range(3):
            bits = vote_round(agg, 1, D, 50 + rnd)
            a = S.vote(bits, N, ETA, S.MAJORITY, 1, None if g1 is None else S.widen(g1, okind))[0]
            g1 = S.round_out((a + F32(sd) * fa.noise_host(seed, 1, rnd, 0, N)).astype(F32), okind)
            S.assert_bits(agg.finalize(1), g1, "noise, round %d" % rnd)
            bits = vote_round(agg, 2, D, 60 + rnd)
            a = S.vote(bits, N, ETA, S.MEAN, 1, None if g2 is None else S.widen(g2, okind))[0]
            state = SO.bootstrap(SO.ADAM, a) if state is None else SO.step(SO.ADAM, a, *state, **hp)
            g2 = S.round_out(state[0], okind)
            S.assert_bits(agg.finalize(2), g2, "server optimizer, round %d" % rnd)


def refused(fa, code, fn, *args, **kw):
    with pytest.raises(fa.FaError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, ei.value


def test_refusals(fa, torch_gpu):
    D = 5
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_ARG, agg.set_sign, 1, ETA)  # an rs context
    others = {"clip": lambda a, p: a.set_clip(1.0, p), "krum": lambda a, p: a.set_krum(1, None, p),
              "dnc": lambda a, p: a.set_dnc(1, 8, p), "geomed": lambda a, p: a.set_geomed(4, 1e-6, p),
              "secagg": lambda a, p: a.set_secagg(1.0, p), "mx8": lambda a, p: a.set_mx8(True, p),
              "topk": lambda a, p: a.set_topk(16, p), "rot1": lambda a, p: a.set_rot1(True, p),
              "lowrank": lambda a, p: a.set_lowrank(p, [(0, 100, 200)], 2)}
    with fa.Aggregator(1) as agg:
        for i, (name, setter) in enumerate(others.items()):  # every excluded stage and format, in both call orders
            agg.define(10 + i, N, fa.F32, fa.F32, D)
            agg.set_sign(10 + i, ETA)
            refused(fa, fa.ERR_ARG, setter, agg, 10 + i)
            agg.define(30 + i, N, fa.F32, fa.F32, D)
            setter(agg, 30 + i)
            refused(fa, fa.ERR_ARG, agg.set_sign, 30 + i, ETA)
        agg.define(50, N, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        refused(fa, fa.ERR_ARG, agg.set_sign, 50, ETA)  # Bulyan's kind of part
        refused(fa, fa.ERR_ARG, agg.set_sign, -1, ETA)  # no context default
        # the planes: not under the mean rule, not with noise or a server optimizer, in either order
        agg.define(60, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_STATE, agg.set_sign, 60, ETA, S.MEAN, 1, True)
        agg.set_sign(60, ETA, planes=True)
        refused(fa, fa.ERR_STATE, agg.set_noise, 0.5, 1, 60)
        refused(fa, fa.ERR_STATE, agg.set_server_opt, SO.ADAM, 0.5, part_id=60)
        refused(fa, fa.ERR_STATE, agg.copy_sign_planes, 60)  # no reducing call yet
        for i, first in enumerate((lambda p: agg.set_noise(0.5, 1, p), lambda p: agg.set_server_opt(SO.ADAM, 0.5, part_id=p))):
            agg.define(61 + i, N, fa.F32, fa.F32, D)
            first(61 + i)
            refused(fa, fa.ERR_STATE, agg.set_sign, 61 + i, ETA, S.MAJORITY, 1, True)
            agg.set_sign(61 + i, ETA)  # without planes the stages compose
        # receipts: a dense submit, a sign submit to a part without the stage, a slot missing at the reducing call
        refused(fa, fa.ERR_STATE, agg.submit, 60, 0, np.zeros(N, F32))
        agg.define(70, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_STATE, agg.submit_sign, 70, 0, np.zeros(S.words(N), np.uint32))
        for k in range(D - 1):
            agg.submit_sign(60, k, np.zeros(S.words(N), np.uint32))
        refused(fa, fa.ERR_STATE, agg.reduce, 60)
        refused(fa, fa.ERR_STATE, agg.finalize, 60)
        refused(fa, fa.ERR_ARG, agg.set_sign, 60, ETA, S.MAJORITY, D + 1)  # the margin against the part's D
