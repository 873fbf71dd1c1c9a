"""GPU: the sparse-sum stage through Aggregator (fa_set_sparse_sum, fa_submit_sparse) against tests/sparse_ref.py, every
bit: a bootstrap (absolute) round and two rounds against the part's output on one GPU, two range shards, range pieces and
an FA_ACCUMULATE_ON_ARRIVAL context, the last round after another k_max and with a receipt from pinned memory; noise, a server optimizer and an MX8 reply behind the stage; fa_reduce_parts; the refusals; a bad idx."""
import numpy as np
import pytest

import mx8_reply_ref as P
import server_opt_ref as SO
import sparse_ref as S

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
N, K = 20000 + 37, 2500
LAYOUTS = {
    "one GPU": lambda fa: fa.Aggregator(1),
    "two shards": lambda fa: fa.Aggregator(devices=[0, 0], shared_device=True),
    "pieces": lambda fa: fa.Aggregator(1),
    "eager": lambda fa: fa.Aggregator(1, eager=True),
}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "bf16": fa.BF16, "f16": fa.F16}[kind]


def sparse_round(agg, part, D, seed, pin=None):
    """Submits D receipts (client 1 an empty one) under mixed-sign weights; returns (idx, val, w).  pin(nbytes): a
    PinnedBuffer that the caller keeps; client 0 then submits from two of them under FA_HOST_PINNED."""
    idx, val = S.receipts(D, N, K, seed, empty={1})
    w = (np.random.default_rng(seed).uniform(0.5, 1.5, D) * np.where(np.arange(D) % 3, 1.0, -1.0)).astype(F32)
    for c in range(D):
        i, v = idx[c], val[c]
        if pin and c == 0:
            i, v = pin(i.nbytes).view(U32), pin(v.nbytes).view(F32)
            i[:], v[:] = idx[c], val[c]
        agg.submit_sparse(part, c, i, v, w[c], pinned=bool(pin and c == 0))
    return idx, val, w


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("D,okind", [(5, "f32"), (8, "bf16"), (3, "f16")])
def test_three_rounds(fa, torch_gpu, D, okind, layout):
    part = 3
    with LAYOUTS[layout](fa) as agg:
        if layout == "pieces":
            agg.set_tuning(piece_span_kib=64, piece_split_kib=-1)
        agg.define(part, N, fa.F32, fa_dt(fa, okind), D)
        if layout == "pieces":
            assert len(agg.pieces(part, 0, 0)) >= 2
        agg.set_sparse_sum(part, K)
        g, pins = None, []  # the bootstrap round is absolute; then the reference is the previous output
        for rnd in range(3):
            if rnd == 2:  # another k_max: new shadows, the round under way dropped, the reference kept (rule 4)
                agg.submit_sparse(part, 0, np.zeros(1, U32), np.ones(1, F32))
                agg.set_sparse_sum(part, 2 * K)
                assert agg.progress(part)[0] == 0
            pin = (lambda b: pins.append(fa.PinnedBuffer(b)) or pins[-1]) if rnd == 2 else None
            idx, val, w = sparse_round(agg, part, D, 10 * D + rnd, pin)
            if rnd == 1:
                agg.reduce_parts([part])  # as for any stage part: the finalize then only copies out
            out = agg.finalize(part)
            a = S.sparse_sum(idx, val, w, N, 0, None if g is None else S.widen(g, okind))
            S.assert_bits(out, S.round_out(a, okind), "round %d, %s" % (rnd, layout))
            g = out


@pytest.mark.parametrize("okind", ["f32", "bf16"])
def test_noise_optimizer_and_reply_follow(fa, torch_gpu, okind):
    D, hp, sd, seed = 5, dict(lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3), 0.25, 77
    owners = P.Owners(okind)
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa_dt(fa, okind), D)
        agg.set_sparse_sum(1, K)
        agg.set_noise(sd, seed, 1)
        agg.define(2, N, fa.F32, fa_dt(fa, okind), D)
        agg.set_server_opt(SO.ADAM, part_id=2, **hp)
        agg.set_sparse_sum(2, K)
        agg.define(3, N, fa.F32, fa_dt(fa, okind), D)
        agg.set_sparse_sum(3, K)
        agg.set_mx8_reply(True, 3)
        g1 = g2 = g3 = state = None
        for rnd in range(3):
            idx, val, w = sparse_round(agg, 1, D, 50 + rnd)
            a = S.sparse_sum(idx, val, w, N, 0, None if g1 is None else S.widen(g1, okind))
            g1 = S.round_out((a + F32(sd) * fa.noise_host(seed, 1, rnd, 0, N)).astype(F32), okind)
            S.assert_bits(agg.finalize(1), g1, "noise, round %d" % rnd)
            idx, val, w = sparse_round(agg, 2, D, 60 + rnd)
            a = S.sparse_sum(idx, val, w, N, 0, None if g2 is None else S.widen(g2, okind))
            state = SO.bootstrap(SO.ADAM, a) if state is None else SO.step(SO.ADAM, a, *state, **hp)
            g2 = S.round_out(state[0], okind)
            S.assert_bits(agg.finalize(2), g2, "server optimizer, round %d" % rnd)
            idx, val, w = sparse_round(agg, 3, D, 70 + rnd)
            y = S.round_out(S.sparse_sum(idx, val, w, N, 0, None if g3 is None else S.widen(g3, okind)), okind)
            want = owners.round(y)  # (q, e, g'): from the second round on the owners hold g', and so does the part
            g3 = y if rnd == 0 else want[2]
            S.assert_bits(agg.finalize(3), g3, "mx8 reply, round %d" % rnd)
            if rnd:
                q, e = agg.copy_mx8(3)
                assert np.array_equal(q, want[0]) and np.array_equal(e, want[1]), "codes, round %d" % rnd


def refused(fa, code, fn, *args, **kw):
    with pytest.raises(fa.FaError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_refusals(fa, torch_gpu):
    D = 5
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_ARG, agg.set_sparse_sum, 1, K)  # an rs context
    others = {"clip": lambda a, p: a.set_clip(1.0, p), "krum": lambda a, p: a.set_krum(1, None, p),
              "dnc": lambda a, p: a.set_dnc(1, 8, p), "geomed": lambda a, p: a.set_geomed(4, 1e-6, p),
              "secagg": lambda a, p: a.set_secagg(1.0, p), "sign": lambda a, p: a.set_sign(p, 0.01),
              "mx8": lambda a, p: a.set_mx8(True, p), "topk": lambda a, p: a.set_topk(16, p),
              "rot1": lambda a, p: a.set_rot1(True, p), "lowrank": lambda a, p: a.set_lowrank(p, [(0, 100, 200)], 2)}
    with fa.Aggregator(1) as agg:
        for i, (name, setter) in enumerate(others.items()):  # every excluded stage and format, in both call orders
            agg.define(10 + i, N, fa.F32, fa.F32, D)
            agg.set_sparse_sum(10 + i, K)
            refused(fa, fa.ERR_ARG, setter, agg, 10 + i)
            agg.define(30 + i, N, fa.F32, fa.F32, D)
            setter(agg, 30 + i)
            refused(fa, fa.ERR_ARG, agg.set_sparse_sum, 30 + i, K)
        agg.define(50, N, fa.F32, fa.F32, D, mode=fa.TRIMMED)
        refused(fa, fa.ERR_ARG, agg.set_sparse_sum, 50, K)
        refused(fa, fa.ERR_ARG, agg.set_sparse_sum, -1, K)  # no context default
        agg.define(51, N, fa.F32, fa.F32, 129)
        refused(fa, fa.ERR_ARG, agg.set_sparse_sum, 51, K)  # FA_SPARSE_MAX_CLIENTS
        # receipts: a dense submit, a sparse submit to a part without the stage, too many entries, a slot missing
        agg.define(60, N, fa.F32, fa.F32, D)
        agg.set_sparse_sum(60, K)
        refused(fa, fa.ERR_STATE, agg.submit, 60, 0, np.zeros(N, F32))
        agg.define(70, N, fa.F32, fa.F32, D)
        refused(fa, fa.ERR_STATE, agg.submit_sparse, 70, 0, np.zeros(1, U32), np.zeros(1, F32))
        refused(fa, fa.ERR_ARG, agg.submit_sparse, 60, 0, np.arange(K + 1, dtype=U32), np.zeros(K + 1, F32))
        for c in range(D - 1):
            agg.submit_sparse(60, c, np.zeros(1, U32), np.ones(1, F32))
        refused(fa, fa.ERR_STATE, agg.reduce, 60)
        refused(fa, fa.ERR_STATE, agg.finalize, 60)


def test_a_bad_idx_leaves_the_round_as_it_was(fa, torch_gpu):
    D = 3
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        agg.set_sparse_sum(1, K)
        idx, val, w = sparse_round(agg, 1, D, 5)
        assert "idx[2]" in refused(fa, fa.ERR_ARG, agg.submit_sparse, 1, 0, np.array([4, 9, 9], U32), np.ones(3, F32))
        assert "idx[1]" in refused(fa, fa.ERR_ARG, agg.submit_sparse, 1, 2, np.array([4, N], U32), np.ones(2, F32))
        assert agg.progress(1)[0] == D
        S.assert_bits(agg.finalize(1), S.sparse_sum(idx, val, w, N), "after the refused receipts")
