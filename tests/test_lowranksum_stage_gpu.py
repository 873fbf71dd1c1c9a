"""GPU: the low-rank-sum stage through Aggregator against tests/lowranksum_ref.py, every bit on lattice data: two rounds
(absolute, then against the first output) on one GPU, on two range shards and with pieces forced -- the cuts fall inside
matrices; noise and a server optimizer behind it; the refusals; the removal."""
import numpy as np
import pytest

import lowrank_ref as L
import lowranksum_ref as R
import server_opt_ref as SO
from test_mx8_gpu import fa_dt
from test_sparse_stage_gpu import refused

pytestmark = pytest.mark.gpu

F32 = np.float32
MATS, N = L.bucket()
RANKS, R_MAX = (3, 5, 1, 64, 2), 64
D = len(RANKS)
LAYOUTS = {"one GPU": dict(n_gpus=1), "two shards": dict(devices=[0, 0], shared_device=True), "pieces": dict(n_gpus=1)}


def lr_round(agg, part, seed):
    """Submits D lattice receipts under weights from {1/8 .. 8/8}; returns (fs, w)."""
    fs = [L.lattice(MATS, N, r, seed + c) for c, r in enumerate(RANKS)]
    w = ((np.arange(D) * 3 + seed) % 8 + 1).astype(F32) / 8
    R.assert_exact(fs, RANKS, w, MATS, N)
    for c in range(D):
        agg.submit_lowrank_sum(part, c, fs[c], RANKS[c], w[c])
    return fs, w


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("okind", ["f32", "bf16"])
def test_two_rounds(fa, torch_gpu, okind, layout):
    with fa.Aggregator(**LAYOUTS[layout]) as agg:
        if layout == "pieces":
            agg.set_tuning(piece_span_kib=1, piece_split_kib=-1)
        agg.define(3, N, fa.F32, fa_dt(fa, okind), D)
        if layout == "pieces":
            assert len(agg.pieces(3, 0, 0)) >= 2
        agg.set_lowrank_sum(3, MATS, R_MAX)
        g = None  # the bootstrap round is absolute; then the reference is the previous output
        for rnd in range(2):
            fs, w = lr_round(agg, 3, 10 + rnd)
            out = agg.finalize(3)
            a = R.lowrank_sum(fs, RANKS, w, MATS, N, None if g is None else R.widen(g, okind))
            R.assert_bits(out, R.round_out(a, okind), "round %d, %s" % (rnd, layout))
            g = out


def test_noise_and_optimizer_follow(fa, torch_gpu):
    hp, sd, seed = dict(lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3), 0.25, 77
    with fa.Aggregator(1) as agg:
        for part in (1, 2):
            agg.define(part, N, fa.F32, fa.F32, D)
            agg.set_lowrank_sum(part, MATS, R_MAX)
        agg.set_noise(sd, seed, 1)
        agg.set_server_opt(SO.ADAM, part_id=2, **hp)
        g1 = g2 = state = None
        for rnd in range(2):
            fs, w = lr_round(agg, 1, 50 + rnd)
            a = R.lowrank_sum(fs, RANKS, w, MATS, N, g1)
            g1 = (a + F32(sd) * fa.noise_host(seed, 1, rnd, 0, N)).astype(F32)
            R.assert_bits(agg.finalize(1), g1, "noise, round %d" % rnd)
            fs, w = lr_round(agg, 2, 60 + rnd)
            a = R.lowrank_sum(fs, RANKS, w, MATS, N, g2)
            state = SO.bootstrap(SO.ADAM, a) if state is None else SO.step(SO.ADAM, a, *state, **hp)
            g2 = state[0]
            R.assert_bits(agg.finalize(2), g2, "server optimizer, round %d" % rnd)


def test_refusals_and_removal(fa, torch_gpu, O):
    f = L.lattice(MATS, N, 2, 0)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_ARG, agg.set_lowrank_sum, 1, MATS, R_MAX)  # an rs context
    others = {"clip": lambda a, p: a.set_clip(1.0, p), "krum": lambda a, p: a.set_krum(1, None, p),
              "dnc": lambda a, p: a.set_dnc(1, 8, p), "geomed": lambda a, p: a.set_geomed(4, 1e-6, p),
              "secagg": lambda a, p: a.set_secagg(1.0, p), "sign": lambda a, p: a.set_sign(p, 0.01),
              "sparse": lambda a, p: a.set_sparse_sum(p, 16), "mx8sum": lambda a, p: a.set_mx8_sum(True, p),
              "mx8": lambda a, p: a.set_mx8(True, p), "topk": lambda a, p: a.set_topk(16, p),
              "rot1": lambda a, p: a.set_rot1(True, p), "lowrank": lambda a, p: a.set_lowrank(p, MATS, 2)}
    with fa.Aggregator(1) as agg:
        for i, (name, setter) in enumerate(others.items()):  # every family member and receipt format, in both call orders
            agg.define(10 + i, N, fa.F32, fa.F32, D)
            agg.set_lowrank_sum(10 + i, MATS, R_MAX)
            refused(fa, fa.ERR_ARG, setter, agg, 10 + i)
            agg.define(30 + i, N, fa.F32, fa.F32, D)
            setter(agg, 30 + i)
            refused(fa, fa.ERR_ARG, agg.set_lowrank_sum, 30 + i, MATS, R_MAX)
        agg.define(50, N, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        refused(fa, fa.ERR_ARG, agg.set_lowrank_sum, 50, MATS, R_MAX)
        refused(fa, fa.ERR_ARG, agg.set_lowrank_sum, -1, MATS, R_MAX)  # no context default
        agg.define(51, N, fa.F32, fa.F32, 129)
        refused(fa, fa.ERR_ARG, agg.set_lowrank_sum, 51, MATS, R_MAX)  # FA_LOWRANK_SUM_MAX_CLIENTS
        agg.define(60, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_ARG, agg.set_lowrank_sum, 60, MATS, 65)
        refused(fa, fa.ERR_ARG, agg.set_lowrank_sum, 60, [(0, N, 2)], 2)  # a table beyond the bucket
        refused(fa, fa.ERR_STATE, agg.submit_lowrank_sum, 60, 0, f, 2)  # the part has no stage yet
        agg.set_lowrank_sum(60, MATS, 2)
        refused(fa, fa.ERR_STATE, agg.submit, 60, 0, np.zeros(N, F32))
        refused(fa, fa.ERR_ARG, agg.submit_lowrank_sum, 60, 0, f, 3)  # beyond r_max
        refused(fa, fa.ERR_ARG, agg.submit_lowrank_sum, 60, 0, f[:-1], 2)
        for c in range(D - 1):
            agg.submit_lowrank_sum(60, c, f, 2)
        refused(fa, fa.ERR_STATE, agg.finalize, 60)
        # without the stage the part reduces dense receipts again
        agg.set_lowrank_sum(60, [], 0)
        xs, w = list(np.random.default_rng(3).standard_normal((D, N)).astype(F32)), O.weights(D)
        for c in range(D):
            agg.submit(60, c, xs[c], w[c])
        R.assert_bits(agg.finalize(60), O.fedavg(xs, w), "stage removed")
