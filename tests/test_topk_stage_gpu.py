"""GPU: top-k receipts through a context (fa_set_topk, fa_submit_topk).

One part of n = 3 T + 5 elements (T = 4096, the kernels' tile) and three owners.  A dense round sets the reference; in
the second round every owner sends top-k -- one relative, one absolute, one with no entries -- and the output must be,
bit for bit, that of a twin context given the dense expansions (tests/topk_ref.py) through fa.submit: on one GPU and
on two range shards of one device.  Then the refusals, which leave the round intact, and a part that takes one MX8 and
one top-k receipt."""
import numpy as np
import pytest

import mx8_ref as M
import topk_ref as K

pytestmark = pytest.mark.gpu

F32 = np.float32
N, D, K_MAX = 3 * 4096 + 5, 3, 600
LAYOUTS = {
    "one GPU": lambda fa: fa.Aggregator(1),
    "two shards": lambda fa: fa.Aggregator(devices=[0, 0], shared_device=True),
}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "bf16": fa.BF16}[kind]


def first_round(fa, agg, part, kind, mx8=False):
    agg.define(part, N, fa_dt(fa, kind), fa_dt(fa, kind), D)
    agg.set_topk(K_MAX, part)
    if mx8:
        agg.set_mx8(True, part)
    rng = np.random.default_rng(1)
    for k in range(D):
        agg.submit(part, k, K.round_out(rng.uniform(-1, 1, N).astype(F32), kind), 1.0 + k)
    return agg.finalize(part)


def owner_entries(g, kind, seed, k):
    rng = np.random.default_rng(seed)
    return K.select((F32(0.05) * rng.standard_normal(N).astype(F32)), k)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_second_round_from_topk_receipts(fa, torch_gpu, kind, layout):
    part = 2
    with LAYOUTS[layout](fa) as agg, LAYOUTS[layout](fa) as twin:
        g = first_round(fa, agg, part, kind)
        K.assert_bits(first_round(fa, twin, part, kind), g, "round 1")
        sends = [owner_entries(g, kind, 10, K_MAX) + (False,), owner_entries(g, kind, 11, K_MAX // 2) + (True,),
                 (np.zeros(0, np.uint32), np.zeros(0, F32), False)]
        # the refusals come first and leave the round as it was
        with pytest.raises(fa.FaError) as ei:
            agg.submit_topk(part, 0, *owner_entries(g, kind, 12, K_MAX + 1))
        assert ei.value.code == fa.ERR_ARG and "at most" in str(ei.value)
        bad = sends[0][0].copy()
        bad[5] = bad[4]
        with pytest.raises(fa.FaError) as ei:
            agg.submit_topk(part, 0, bad, sends[0][1])
        assert ei.value.code == fa.ERR_ARG and "idx[5]" in str(ei.value)
        assert agg.progress(part) == (0, 0)
        for k, (idx, val, absolute) in enumerate(sends):
            agg.submit_topk(part, k, idx, val, 1.0 + k, absolute=absolute)
            twin.submit(part, k, K.expand(idx, val, N, 0, kind, None if absolute else g, kind), 1.0 + k)
        assert agg.progress(part) == (D, 0)
        K.assert_bits(agg.finalize(part), twin.finalize(part), "round 2, %s" % layout)


def test_a_part_takes_one_receipt_of_each_kind(fa, torch_gpu):
    part = 0
    with fa.Aggregator(1) as agg, fa.Aggregator(1) as twin:
        g = first_round(fa, agg, part, "f32", mx8=True)
        first_round(fa, twin, part, "f32", mx8=True)
        idx, val = owner_entries(g, "f32", 20, K_MAX)
        q, e = M.encode(F32(0.05) * np.random.default_rng(21).standard_normal(N).astype(F32))
        full = np.random.default_rng(22).uniform(-1, 1, N).astype(F32)
        agg.submit_topk(part, 0, idx, val)
        agg.submit_mx8(part, 1, q, e)
        agg.submit(part, 2, full)
        for k, x in enumerate([K.expand(idx, val, N, 0, "f32", g), M.expand(q, e, 0, "f32", g), full]):
            twin.submit(part, k, x)
        K.assert_bits(agg.finalize(part), twin.finalize(part), "mixed receipts")
