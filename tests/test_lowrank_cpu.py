"""CPU: the host side of low-rank receipts (fa.h "Low-rank receipts") against tests/lowrank_ref.py: the length rule,
the decoder on lattice data (every bit, whole bucket and sub-ranges that cut a matrix), the table checks that name the
first bad entry, the plan's size rule and the cnt == 0 probe, which touches no device."""
import numpy as np
import pytest

import lowrank_ref as L

MATS, N = L.bucket()


@pytest.mark.parametrize("r", [1, 3, 4, 5, 64])
def test_length_and_decode_against_the_reference(fa, r):
    assert fa.lowrank_len(MATS, N, r) == L.length(MATS, N, r)
    assert fa.lowrank_len([], N, r) == N
    f = L.lattice(MATS, N, r, r)
    want = L.decode(f, MATS, N, r)
    for idx0, cnt in ((0, N), (MATS[3][0] + 63 * 10 + 20, 3000), (N - 1, 1), (5, 0)):
        L.assert_bits(fa.lowrank_decode(f, MATS, N, r, idx0, cnt), want[idx0:idx0 + cnt], "r %d [%d, +%d)" % (r, idx0, cnt))


def test_shapes_make_a_table_and_the_encoder_a_receipt(fa):
    mats, n = fa.lowrank_mats([(8, 3, 2, 2), (8,), (5, 6), (2, 2)], min_elems=5)
    assert n == 96 + 8 + 30 + 4 and mats.tolist() == [(0, 8, 12), (104, 5, 6)]
    rng = np.random.default_rng(0)
    delta = rng.standard_normal(n).astype(np.float32)
    low = rng.standard_normal((8, 2)) @ rng.standard_normal((2, 12))  # a rank-2 block is recovered at r = 2
    delta[:96] = low.reshape(-1)
    f = fa.lowrank_encode(delta, mats, 2)
    assert f.dtype == np.float32 and f.size == fa.lowrank_len(mats, n, 2)
    d = fa.lowrank_decode(f, mats, n, 2)
    assert np.allclose(d[:96], delta[:96], atol=1e-5) and np.array_equal(d[96:104], delta[96:104])
    assert np.array_equal(d[134:], delta[134:])


@pytest.mark.parametrize("mats, word", [([(0, 4, 4), (10, 2, 3)], "overlaps"), ([(0, 4, 4), (16, 5, 5)], "beyond"),
                                        ([(20, 2, 2), (3, 2, 2)], "ascend"), ([(0, 2, 2), (8, 0, 3)], "no rows")])
def test_a_bad_table_is_refused_by_its_first_bad_entry(fa, mats, word):
    for call in (lambda: fa.lowrank_check(mats, 40), lambda: fa.lowrank_len(mats, 40, 2), lambda: fa.lowrank_plan(mats, 40),
                 lambda: fa.lowrank_decode(np.zeros(4, np.float32), mats, 40, 2)):
        with pytest.raises(fa.FaError) as ei:
            call()
        assert ei.value.code == fa.ERR_ARG and "matrix 1" in str(ei.value) and word in str(ei.value)
    with pytest.raises(fa.FaError) as ei:
        fa.lowrank_len(MATS, N, 65)
    assert ei.value.code == fa.ERR_ARG and "rank" in str(ei.value)


def test_plan_size_and_the_probe(fa):
    tiles = sum(-(-rows // 64) * -(-cols // 64) for _, rows, cols in MATS)
    assert fa.lowrank_plan(MATS, N).size == 32 * (1 + tiles + len(L.GAPS))  # every gap is one chunk
    assert fa.lowrank_plan(MATS, N, 0, 0).size == 32
    inside = MATS[3][0] + 63 * 2  # rows 2 .. 3 of the 65 x 63 matrix: its first row band, no rest
    assert fa.lowrank_plan(MATS, N, inside, 100).size == 32 * 2
    fa.lowrank_expand_device(None, None, 1, 0, None)  # cnt == 0: no device, FA_OK
    with pytest.raises(fa.FaError) as ei:
        fa.lowrank_expand_device(None, None, 1, 0, None, dst_dtype=fa.BF16, ref_dtype=fa.F16)
    assert ei.value.code == fa.ERR_ARG
