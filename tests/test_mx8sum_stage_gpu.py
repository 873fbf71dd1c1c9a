"""GPU: the MX8-sum stage through Aggregator against tests/mx8sum_ref.py, every bit: three rounds on one GPU, two range shards
and range pieces; noise, a server optimizer and an MX8 reply behind it; the identity with the expanded route; the refusals."""
import numpy as np
import pytest

import mx8_reply_ref as P
import mx8sum_ref as M
import server_opt_ref as SO
from test_mx8_gpu import fa_dt
from test_sparse_stage_gpu import refused

pytestmark = pytest.mark.gpu

F32 = np.float32
N, D = 64 * 5 + 7, 5
LAYOUTS = {"one GPU": dict(n_gpus=1), "two shards": dict(devices=[0, 0], shared_device=True), "pieces": dict(n_gpus=1)}


def mx8_round(agg, part, seed, submit=None, **kw):
    """Submits D receipts of ordinary scales under mixed-sign weights; returns (q, e, w)."""
    q, e = M.receipts(D, N, 0, seed, edges=False)
    w = (np.random.default_rng(seed).uniform(0.5, 1.5, D) * np.where(np.arange(D) % 3, 1.0, -1.0)).astype(F32)
    for c in range(D):
        (submit or agg.submit_mx8_sum)(part, c, q[c], e[c], w[c], **kw)
    return q, e, w


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("okind", ["f32", "bf16", "f16"])
def test_three_rounds(fa, torch_gpu, okind, layout):
    with fa.Aggregator(**LAYOUTS[layout]) as agg:
        if layout == "pieces":
            agg.set_tuning(piece_span_kib=1, piece_split_kib=-1)
        agg.define(3, N, fa.F32, fa_dt(fa, okind), D)
        if layout == "pieces":
            assert len(agg.pieces(3, 0, 0)) >= 2
        agg.set_mx8_sum(True, 3)
        g = None  # the bootstrap round is absolute; then the reference is the previous output
        for rnd in range(3):
            q, e, w = mx8_round(agg, 3, 10 + rnd)
            if rnd == 1:
                agg.reduce_parts([3])  # as for any stage part: the finalize then only copies out
            out = agg.finalize(3)
            a = M.mx8_sum(q, e, w, 0, None if g is None else M.widen(g, okind))
            M.assert_bits(out, M.round_out(a, okind), "round %d, %s" % (rnd, layout))  # the same bits on every layout
            g = out


@pytest.mark.parametrize("okind", ["f32", "bf16"])
def test_noise_optimizer_and_reply_follow(fa, torch_gpu, okind):
    hp, sd, seed = dict(lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3), 0.25, 77
    owners = P.Owners(okind)
    with fa.Aggregator(1) as agg:
        for part in (1, 2, 3):
            agg.define(part, N, fa.F32, fa_dt(fa, okind), D)
            agg.set_mx8_sum(True, part)
        agg.set_noise(sd, seed, 1)
        agg.set_server_opt(SO.ADAM, part_id=2, **hp)
        agg.set_mx8_reply(True, 3)
        g1 = g2 = g3 = state = None
        for rnd in range(3):
            q, e, w = mx8_round(agg, 1, 50 + rnd)
            a = M.mx8_sum(q, e, w, 0, None if g1 is None else M.widen(g1, okind))
            g1 = M.round_out((a + F32(sd) * fa.noise_host(seed, 1, rnd, 0, N)).astype(F32), okind)
            M.assert_bits(agg.finalize(1), g1, "noise, round %d" % rnd)
            q, e, w = mx8_round(agg, 2, 60 + rnd)
            a = M.mx8_sum(q, e, w, 0, None if g2 is None else M.widen(g2, okind))
            state = SO.bootstrap(SO.ADAM, a) if state is None else SO.step(SO.ADAM, a, *state, **hp)
            g2 = M.round_out(state[0], okind)
            M.assert_bits(agg.finalize(2), g2, "server optimizer, round %d" % rnd)
            q, e, w = mx8_round(agg, 3, 70 + rnd)
            y = M.round_out(M.mx8_sum(q, e, w, 0, None if g3 is None else M.widen(g3, okind)), okind)
            want = owners.round(y)  # (q, e, g'): from the second round on the owners hold g', and so does the part
            g3 = y if rnd == 0 else want[2]
            M.assert_bits(agg.finalize(3), g3, "mx8 reply, round %d" % rnd)
            if rnd:
                rq, re = agg.copy_mx8(3)
                assert np.array_equal(rq, want[0]) and np.array_equal(re, want[1]), "codes, round %d" % rnd


def test_absolute_round_is_the_expanded_route(fa, torch_gpu):
    """Rule 5: the same receipts through fa_set_mx8 with FA_MX8_ABSOLUTE into f32 slots and the chain give the same bytes."""
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        agg.set_mx8_sum(True, 1)
        agg.define(2, N, fa.F32, fa.F32, D)
        agg.set_mx8(True, 2)
        mx8_round(agg, 1, 5)
        mx8_round(agg, 2, 5, submit=agg.submit_mx8, absolute=True)
        M.assert_bits(agg.finalize(1), agg.finalize(2), "absolute round")


def test_refusals(fa, torch_gpu, O):
    q, e = M.receipts(1, N, 0, 1)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_ARG, agg.set_mx8_sum, True, 1)  # an rs context
    others = {"clip": lambda a, p: a.set_clip(1.0, p), "krum": lambda a, p: a.set_krum(1, None, p),
              "dnc": lambda a, p: a.set_dnc(1, 8, p), "geomed": lambda a, p: a.set_geomed(4, 1e-6, p),
              "secagg": lambda a, p: a.set_secagg(1.0, p), "sign": lambda a, p: a.set_sign(p, 0.01),
              "sparse": lambda a, p: a.set_sparse_sum(p, 16), "mx8": lambda a, p: a.set_mx8(True, p),
              "topk": lambda a, p: a.set_topk(16, p), "rot1": lambda a, p: a.set_rot1(True, p),
              "lowrank": lambda a, p: a.set_lowrank(p, [(0, 10, 20)], 2)}
    with fa.Aggregator(1) as agg:
        for i, (name, setter) in enumerate(others.items()):  # every family member and receipt format, in both call orders
            agg.define(10 + i, N, fa.F32, fa.F32, D)
            agg.set_mx8_sum(True, 10 + i)
            refused(fa, fa.ERR_ARG, setter, agg, 10 + i)
            agg.define(30 + i, N, fa.F32, fa.F32, D)
            setter(agg, 30 + i)
            refused(fa, fa.ERR_ARG, agg.set_mx8_sum, True, 30 + i)
        agg.define(50, N, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        refused(fa, fa.ERR_ARG, agg.set_mx8_sum, True, 50)
        refused(fa, fa.ERR_ARG, agg.set_mx8_sum, True, -1)  # no context default
        agg.define(51, N, fa.F32, fa.F32, 129)
        refused(fa, fa.ERR_ARG, agg.set_mx8_sum, True, 51)  # FA_MX8_SUM_MAX_CLIENTS
        agg.define(60, N, fa.F32, fa.F32, D)
        agg.set_mx8_sum(True, 60)
        refused(fa, fa.ERR_STATE, agg.submit, 60, 0, np.zeros(N, F32))
        agg.define(70, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_STATE, agg.submit_mx8_sum, 70, 0, q[0], e[0])
        for c in range(D - 1):
            agg.submit_mx8_sum(60, c, q[0], e[0])
        refused(fa, fa.ERR_STATE, agg.reduce, 60)
        refused(fa, fa.ERR_STATE, agg.finalize, 60)
        # without the stage the part reduces dense receipts again
        agg.set_mx8_sum(False, 60)
        xs, w = list(np.random.default_rng(3).standard_normal((D, N)).astype(F32)), O.weights(D)
        for c in range(D):
            agg.submit(60, c, xs[c], w[c])
        M.assert_bits(agg.finalize(60), O.fedavg(xs, w), "stage removed")
