"""GPU: low-rank receipts through a context (fa_set_lowrank, fa_submit_lowrank).

One part over lowrank_ref.bucket() with a reference set and four owners: two send low-rank receipts of different rank
(one relative, one absolute), one top-k, one a dense receipt.  On lattice data kernel and decoder agree in every bit,
so the round must equal, bit for bit, that of a twin context given g + fa.lowrank_decode(f) densely: on one GPU, on two
range shards of one device and on a part held in four pieces -- the shard boundary and the piece boundaries fall inside
matrices.  Then the refusals, which leave the round intact.
"""
import numpy as np
import pytest

import lowrank_ref as L
import topk_ref as K

pytestmark = pytest.mark.gpu

F32 = np.float32
MATS, N = L.bucket()
D, R_MAX, K_MAX = 4, 8, 100
LAYOUTS = {
    "one GPU": lambda fa: fa.Aggregator(1),
    "two shards": lambda fa: fa.Aggregator(devices=[0, 0], shared_device=True),
    "pieces": lambda fa: fa.Aggregator(1),
}


def make_part(fa, agg, part, layout, g):
    if layout == "pieces":
        agg.set_tuning(piece_span_kib=32, piece_split_kib=-1)
    agg.define(part, N, fa.F32, fa.F32, D)
    if layout == "pieces":
        assert len(agg.pieces(part, 0, 0)) == 4
    agg.set_lowrank(part, MATS, R_MAX)
    agg.set_topk(K_MAX, part)
    agg.set_mx8_reference(part, g)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_round_from_mixed_receipts(fa, torch_gpu, layout):
    part = 1
    g = (np.random.default_rng(1).integers(-64, 65, N) / 16).astype(F32)
    f3, f8 = L.lattice(MATS, N, 3, 30), L.lattice(MATS, N, R_MAX, 80)
    idx, val = K.select(np.random.default_rng(2).standard_normal(N).astype(F32), K_MAX)
    full = np.random.default_rng(3).uniform(-1, 1, N).astype(F32)
    dense = [g + fa.lowrank_decode(f3, MATS, N, 3), fa.lowrank_decode(f8, MATS, N, R_MAX), K.expand(idx, val, N, 0, "f32", g), full]
    L.assert_bits(dense[0], L.expand(f3, MATS, N, 3, 0, N, "f32", g), "the decoder is the restatement")
    with LAYOUTS[layout](fa) as agg, LAYOUTS[layout](fa) as twin:
        make_part(fa, agg, part, layout, g)
        make_part(fa, twin, part, layout, g)
        # the refusals come first and leave the round as it was
        for args, word in (((f8, R_MAX + 1), "rank"), ((f8, 3), "values"), ((f3[:-1], 3), "values")):
            with pytest.raises(fa.FaError) as ei:
                agg.submit_lowrank(part, 0, *args)
            assert ei.value.code == fa.ERR_ARG and word in str(ei.value)
        assert agg.progress(part) == (0, 0)
        agg.submit_lowrank(part, 0, f3, 3, 1.0)
        f3[:] = 0  # reusable on return: the library took its copy
        agg.submit_lowrank(part, 1, f8, R_MAX, 2.0, absolute=True)
        agg.submit_topk(part, 2, idx, val, 3.0)
        agg.submit(part, 3, full, 4.0)
        for k, x in enumerate(dense):
            twin.submit(part, k, x, 1.0 + k)
        assert agg.progress(part) == (D, 0)
        L.assert_bits(agg.finalize(part), twin.finalize(part), "mixed receipts, %s" % layout)


def test_refusals(fa, torch_gpu):
    f = L.lattice(MATS, N, 2, 0)
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        with pytest.raises(fa.FaError) as ei:
            agg.set_lowrank(1, MATS, R_MAX)
        assert ei.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(ei.value)
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa.F32, D, mode=fa.LITERAL)
        agg.define(2, N, fa.F32, fa.F32, D)
        agg.define(3, N, fa.F32, fa.F32, D)
        agg.set_secagg(2.0 ** -16, 3)
        for part, word in ((1, "FA_LITERAL"), (3, "secagg"), (-1, "context default")):
            with pytest.raises(fa.FaError) as ei:
                agg.set_lowrank(part, MATS, R_MAX)
            assert ei.value.code == fa.ERR_ARG and word in str(ei.value)
        with pytest.raises(fa.FaError) as ei:
            agg.set_lowrank(2, MATS, 65)
        assert ei.value.code == fa.ERR_ARG and "r_max" in str(ei.value)
        with pytest.raises(fa.FaError) as ei:  # the part does not take them yet
            agg.submit_lowrank(2, 0, f, 2, absolute=True)
        assert ei.value.code == fa.ERR_STATE and "fa_set_lowrank" in str(ei.value)
        agg.set_lowrank(2, MATS, R_MAX)
        with pytest.raises(fa.FaError) as ei:  # never reduced, no reference
            agg.submit_lowrank(2, 0, f, 2)
        assert ei.value.code == fa.ERR_STATE and "reference" in str(ei.value)
        agg.submit_lowrank(2, 0, f, 2, absolute=True)  # absolute mode needs none
        assert agg.progress(2) == (1, 0)
        agg.set_lowrank(2, [], 0)  # off again
        with pytest.raises(fa.FaError) as ei:
            agg.submit_lowrank(2, 1, f, 2, absolute=True)
        assert ei.value.code == fa.ERR_STATE
