"""GPU: the rot1-sum stage through Aggregator against tests/rot1sum_ref.py, every bit: an absolute round and relative ones on
one GPU, two range shards and range pieces (cuts inside blocks); noise, a server optimizer and an MX8 reply behind it; the
refusals."""
import numpy as np
import pytest

import mx8_reply_ref as P
import rot1sum_ref as R
import server_opt_ref as SO
from test_mx8_gpu import fa_dt
from test_sparse_stage_gpu import refused

pytestmark = pytest.mark.gpu

F32 = np.float32
N, D = 2 * 4096 + 200, 5
SEEDS = [7, 9, 7, 7, 9]
LAYOUTS = {"one GPU": dict(n_gpus=1), "two shards": dict(devices=[0, 0], shared_device=True), "pieces": dict(n_gpus=1)}


def rot1_round(fa, agg, part, rng_seed):
    """Submits D receipts in two seed groups under mixed-sign weights; returns (bits, scale, w)."""
    bits, scale, _ = R.receipts(fa, D, N, 0, rng_seed, edges=False)
    w = (np.random.default_rng(rng_seed).uniform(0.5, 1.5, D) * np.where(np.arange(D) % 3, 1.0, -1.0)).astype(F32)
    for c in range(D):
        agg.submit_rot1_sum(part, c, bits[c], scale[c], SEEDS[c], w[c])
    return bits, scale, w


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("okind", ["f32", "bf16", "f16"])
def test_three_rounds(fa, torch_gpu, okind, layout):
    with fa.Aggregator(**LAYOUTS[layout]) as agg:
        if layout == "pieces":
            agg.set_tuning(piece_span_kib=1, piece_split_kib=-1)
        agg.define(3, N, fa.F32, fa_dt(fa, okind), D)
        if layout == "pieces":
            assert len(agg.pieces(3, 0, 0)) >= 2
        agg.set_rot1_sum(True, 3)
        g = None  # the bootstrap round is absolute; then the reference is the previous output
        for rnd in range(3):
            bits, scale, w = rot1_round(fa, agg, 3, 10 + rnd)
            if rnd == 1:
                agg.reduce_parts([3])  # as for any stage part: the finalize then only copies out
            out = agg.finalize(3)
            a = R.rot1_sum(fa, bits, scale, SEEDS, w, N, 0, None if g is None else R.widen(g, okind))
            R.assert_bits(out, R.round_out(a, okind), "round %d, %s" % (rnd, layout))  # the same bits on every layout
            g = out


@pytest.mark.parametrize("okind", ["f32", "bf16"])
def test_noise_optimizer_and_reply_follow(fa, torch_gpu, okind):
    hp, sd, seed = dict(lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3), 0.25, 77
    owners = P.Owners(okind)
    with fa.Aggregator(1) as agg:
        for part in (1, 2, 3):
            agg.define(part, N, fa.F32, fa_dt(fa, okind), D)
            agg.set_rot1_sum(True, part)
        agg.set_noise(sd, seed, 1)
        agg.set_server_opt(SO.ADAM, part_id=2, **hp)
        agg.set_mx8_reply(True, 3)
        g1 = g2 = g3 = state = None
        for rnd in range(2):
            bits, scale, w = rot1_round(fa, agg, 1, 50 + rnd)
            a = R.rot1_sum(fa, bits, scale, SEEDS, w, N, 0, None if g1 is None else R.widen(g1, okind))
            g1 = R.round_out((a + F32(sd) * fa.noise_host(seed, 1, rnd, 0, N)).astype(F32), okind)
            R.assert_bits(agg.finalize(1), g1, "noise, round %d" % rnd)
            bits, scale, w = rot1_round(fa, agg, 2, 60 + rnd)
            a = R.rot1_sum(fa, bits, scale, SEEDS, w, N, 0, None if g2 is None else R.widen(g2, okind))
            state = SO.bootstrap(SO.ADAM, a) if state is None else SO.step(SO.ADAM, a, *state, **hp)
            g2 = R.round_out(state[0], okind)
            R.assert_bits(agg.finalize(2), g2, "server optimizer, round %d" % rnd)
            bits, scale, w = rot1_round(fa, agg, 3, 70 + rnd)
            y = R.round_out(R.rot1_sum(fa, bits, scale, SEEDS, w, N, 0, None if g3 is None else R.widen(g3, okind)), okind)
            want = owners.round(y)  # (q, e, g'): from the second round on the owners hold g', and so does the part
            g3 = y if rnd == 0 else want[2]
            R.assert_bits(agg.finalize(3), g3, "mx8 reply, round %d" % rnd)
            if rnd:
                rq, re = agg.copy_mx8(3)
                assert np.array_equal(rq, want[0]) and np.array_equal(re, want[1]), "codes, round %d" % rnd


def test_refusals(fa, torch_gpu, O):
    bits, scale, _ = R.receipts(fa, 1, N, 0, 1)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        assert "FA_SHARD_CLIENT_RS" in refused(fa, fa.ERR_ARG, agg.set_rot1_sum, True, 1)
    others = {"clip": lambda a, p: a.set_clip(1.0, p), "krum": lambda a, p: a.set_krum(1, None, p),
              "dnc": lambda a, p: a.set_dnc(1, 8, p), "geomed": lambda a, p: a.set_geomed(4, 1e-6, p),
              "secagg": lambda a, p: a.set_secagg(1.0, p), "sign": lambda a, p: a.set_sign(p, 0.01),
              "sparse": lambda a, p: a.set_sparse_sum(p, 16), "mx8 sum": lambda a, p: a.set_mx8_sum(True, p),
              "lowrank sum": lambda a, p: a.set_lowrank_sum(p, [(0, 10, 20)], 2), "mx8": lambda a, p: a.set_mx8(True, p),
              "topk": lambda a, p: a.set_topk(16, p), "rot1": lambda a, p: a.set_rot1(True, p),
              "lowrank": lambda a, p: a.set_lowrank(p, [(0, 10, 20)], 2)}
    with fa.Aggregator(1) as agg:
        for i, (name, setter) in enumerate(others.items()):  # every family member and receipt format, in both call orders
            agg.define(10 + i, N, fa.F32, fa.F32, D)
            agg.set_rot1_sum(True, 10 + i)
            assert "rot1-sum stage" in refused(fa, fa.ERR_ARG, setter, agg, 10 + i), name
            agg.define(30 + i, N, fa.F32, fa.F32, D)
            setter(agg, 30 + i)
            assert "stage" in refused(fa, fa.ERR_ARG, agg.set_rot1_sum, True, 30 + i), name
        agg.define(50, N, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        assert "FA_TRIMMED" in refused(fa, fa.ERR_ARG, agg.set_rot1_sum, True, 50)
        assert "context default" in refused(fa, fa.ERR_ARG, agg.set_rot1_sum, True, -1)
        agg.define(51, N, fa.F32, fa.F32, 129)
        assert "129" in refused(fa, fa.ERR_ARG, agg.set_rot1_sum, True, 51)  # FA_ROT1_SUM_MAX_CLIENTS
        agg.define(60, N, fa.F32, fa.F32, D)
        agg.set_rot1_sum(True, 60)
        assert "fa_submit_rot1_sum" in refused(fa, fa.ERR_STATE, agg.submit, 60, 0, np.zeros(N, F32))
        agg.define(70, N, fa.F32, fa.F32, D)
        assert "fa_set_rot1_sum" in refused(fa, fa.ERR_STATE, agg.submit_rot1_sum, 70, 0, bits[0], scale[0], 7)
        for c in range(D - 1):
            agg.submit_rot1_sum(60, c, bits[0], scale[0], 7)
        refused(fa, fa.ERR_STATE, agg.reduce, 60)
        refused(fa, fa.ERR_STATE, agg.finalize, 60)
        # without the stage the part reduces dense receipts again, as a part that never had it
        agg.set_rot1_sum(False, 60)
        xs, w = list(np.random.default_rng(3).standard_normal((D, N)).astype(F32)), O.weights(D)
        for c in range(D):
            agg.submit(60, c, xs[c], w[c])
        R.assert_bits(agg.finalize(60), O.fedavg(xs, w), "stage removed")
