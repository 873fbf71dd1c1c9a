"""GPU: rot1 receipts through a context (fa_set_rot1, fa_submit_rot1).

A dense round sets the reference; in the second one owner sends a relative rot1 receipt, one an absolute one and one a
dense receipt, and the output must be, bit for bit, that of a twin context given the expansions of tests/rot1_ref.py
through fa.submit: on one GPU and on two range shards of one device, whose cut falls inside a block."""
import numpy as np
import pytest

import mx8_ref as M
import rot1_ref as R
import topk_ref as K

pytestmark = pytest.mark.gpu

F32 = np.float32
N, D = 3 * 4096 + 5, 3
LAYOUTS = {
    "one GPU": lambda fa: fa.Aggregator(1),
    "two shards": lambda fa: fa.Aggregator(devices=[0, 0], shared_device=True),
}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "bf16": fa.BF16}[kind]


def first_round(fa, agg, part, kind, setters=("rot1",)):
    agg.define(part, N, fa_dt(fa, kind), fa_dt(fa, kind), D)
    for s in setters:
        getattr(agg, "set_" + s)(600 if s == "topk" else True, part)
    rng = np.random.default_rng(1)
    for k in range(D):
        agg.submit(part, k, R.round_out(rng.uniform(-1, 1, N).astype(F32), kind), 1.0 + k)
    return agg.finalize(part)


def update(seed):
    return F32(0.05) * np.random.default_rng(seed).standard_normal(N).astype(F32)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_second_round_from_rot1_receipts(fa, torch_gpu, kind, layout):
    part = 2
    with LAYOUTS[layout](fa) as agg, LAYOUTS[layout](fa) as twin:
        g = first_round(fa, agg, part, kind)
        R.assert_bits(first_round(fa, twin, part, kind), g, "round 1")
        sends = [R.encode_delta(update(10), 3) + (3, False), R.encode_delta(update(11) + F32(1), 4) + (4, True)]
        dense = R.round_out(np.random.default_rng(12).uniform(-1, 1, N).astype(F32), kind)
        for k, (bits, scale, seed, absolute) in enumerate(sends):
            agg.submit_rot1(part, k, bits, scale, seed, 1.0 + k, absolute=absolute)
            twin.submit(part, k, R.expand(bits, scale, seed, 0, N, kind, None if absolute else g, kind), 1.0 + k)
        agg.submit(part, 2, dense, 3.0)
        twin.submit(part, 2, dense, 3.0)
        assert agg.progress(part) == (D, 0)
        R.assert_bits(agg.finalize(part), twin.finalize(part), "round 2, %s" % layout)


def test_a_part_without_the_format_refuses(fa, torch_gpu):
    part = 1
    with fa.Aggregator(1) as agg:
        first_round(fa, agg, part, "f32", setters=("mx8",))
        bits, scale = R.encode_delta(update(1), 1)
        with pytest.raises(fa.FaError) as ei:
            agg.submit_rot1(part, 0, bits, scale, 1)
        assert ei.value.code == fa.ERR_STATE and "fa_set_rot1" in str(ei.value)
        assert agg.progress(part) == (0, 0)


def test_a_part_takes_one_receipt_of_each_kind(fa, torch_gpu):
    part = 0
    with fa.Aggregator(1) as agg, fa.Aggregator(1) as twin:
        g = first_round(fa, agg, part, "f32", setters=("mx8", "topk", "rot1"))
        first_round(fa, twin, part, "f32", setters=("mx8", "topk", "rot1"))
        idx, val = K.select(update(20), 600)
        q, e = M.encode(update(21))
        bits, scale = R.encode_delta(update(22), 9)
        agg.submit_topk(part, 0, idx, val)
        agg.submit_mx8(part, 1, q, e)
        agg.submit_rot1(part, 2, bits, scale, 9)
        for k, x in enumerate([K.expand(idx, val, N, 0, "f32", g), M.expand(q, e, 0, "f32", g),
                               R.expand(bits, scale, 9, 0, N, "f32", g)]):
            twin.submit(part, k, x)
        R.assert_bits(agg.finalize(part), twin.finalize(part), "mixed receipts")
