"""GPU: fa_lowrank_expand_device (fa.h "Low-rank receipts") against tests/lowrank_ref.py.

The kernel cuts matrices into 64 x 64 tiles of 16 x 16 MFMA blocks, takes the rank in steps of 4 and fills of 32, and
stores runs of 8 elements laid on the slot's 16-byte grid.  The bucket (lowrank_ref.bucket) holds a matrix on every
side of those sizes, rest gaps around them and matrix offsets at every phase; the ranks sit on both sides of a k-step
and span two fills; the ranges cut a matrix in mid-row and mid-tile; slot and reference are aligned, off 16 bytes in
agreement and in disagreement.  On lattice data every sum is exact, so every bit must agree (NaN as NaN).  The slot
lies between guard bands (tests/guarded.py) that must survive.
"""
import functools

import numpy as np
import pytest

import guarded as G
import lowrank_ref as L
from test_mx8_gpu import ITEM, NP_DT, PAIR_IDS, PAIRS, at_phase, fa_dt
from test_topk_gpu import phase_sets

pytestmark = pytest.mark.gpu

F32 = np.float32
MATS, N = L.bucket()
WIDE = MATS[3][0]  # the 65 x 63 matrix: two row bands
# the whole bucket; from mid-row 10 of the first band into the second; inside the second column tile of the 7 x 130
RANGES = [(0, N), (WIDE + 63 * 10 + 20, 3000), (MATS[5][0] + 130 * 2 + 70, 500)]


@functools.lru_cache(maxsize=None)
def receipt(r):
    f = L.lattice(MATS, N, r, r)
    return f, L.decode(f, MATS, N, r)


def run_kernel(fa, torch, f, r, idx0, cnt, slot_kind, g=None, ref_kind=None, dp=0, rp=0, what=""):
    """One launch into a guarded slot at element phase dp, the reference at rp: the slot's elements."""
    plan = at_phase(torch, fa.lowrank_plan(MATS, N, idx0, cnt), 0)[1]
    f_v = at_phase(torch, f, 4)[1]
    r_v = at_phase(torch, g, rp * ITEM[ref_kind])[1] if ref_kind else None
    snap = G.snapshot(r_v) if ref_kind else None
    buf = G.GuardedBuf(torch, cnt * ITEM[slot_kind], dp * ITEM[slot_kind])
    fa.lowrank_expand_device(plan, f_v, r, cnt, buf.ptr, fa_dt(fa, slot_kind), ref=r_v, ref_dtype=fa_dt(fa, ref_kind),
                             idx0=idx0)
    torch.cuda.synchronize()
    buf.check(what)
    if ref_kind:
        G.assert_unchanged(r_v, snap, what)
    return buf.payload().cpu().numpy().view(NP_DT[slot_kind]).copy()


@pytest.mark.parametrize("r", [1, 3, 4, 5, 64])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_lattice_receipts_expand_bit_for_bit(fa, torch_gpu, pair, r):
    slot_kind, ref_kind = pair
    f, _ = receipt(r)
    ref = L.round_out(np.random.default_rng(7).uniform(-1, 1, N).astype(F32), ref_kind) if ref_kind else None
    for idx0, cnt in RANGES:
        g = ref[idx0:idx0 + cnt] if ref_kind else None
        want = L.expand(f, MATS, N, r, idx0, cnt, slot_kind, g, ref_kind)
        for dp, rp in phase_sets(slot_kind, ref_kind):
            what = "%s r %d [%d, +%d) phases dst%d ref%d" % (PAIR_IDS[PAIRS.index(pair)], r, idx0, cnt, dp, rp)
            L.assert_bits(run_kernel(fa, torch_gpu, f, r, idx0, cnt, slot_kind, g, ref_kind, dp, rp, what), want, what)


def test_random_factors_stay_inside_the_rule_s_bound(fa, torch_gpu):
    """|x - S| <= 2^-24 |S| + r 2^-52 sum |p q| + 2^-150: one rounding of a sum whose adds came in any order."""
    r = 64
    f = np.random.default_rng(3).standard_normal(L.length(MATS, N, r)).astype(F32)
    S, A = L.sums(f, MATS, N, r)
    x = run_kernel(fa, torch_gpu, f, r, 0, N, "f32").astype(np.float64)
    bound = 2.0 ** -24 * np.abs(S) + r * 2.0 ** -52 * A + 2.0 ** -150
    worst = np.max(np.abs(x - S) - bound)
    assert worst <= 0, "beyond the bound by %g at element %d" % (worst, int(np.argmax(np.abs(x - S) - bound)))


def test_a_nan_reaches_its_row_and_an_inf_its_column_only(fa, torch_gpu):
    r = 5
    f = receipt(r)[0].copy()
    P, Q = L.factors(f, MATS, r)[0][3]
    P[3, 0], Q[5, 4] = np.nan, np.inf
    x = run_kernel(fa, torch_gpu, f, r, 0, N, "f32")
    bad = np.zeros((65, 63), bool)
    bad[3, :], bad[:, 5] = True, True
    want = np.zeros(N, bool)
    want[WIDE:WIDE + 65 * 63] = bad.reshape(-1)
    assert np.array_equal(~np.isfinite(x), want)
    L.assert_bits(x, L.decode(f, MATS, N, r), "non-finite factors")


def test_refusals_on_the_device(fa, torch_gpu):
    t = torch_gpu.zeros(64, dtype=torch_gpu.float32, device="cuda")
    for kw, code in ((dict(dst=t.data_ptr() + 2), fa.ERR_ALIGN), (dict(f=t.data_ptr() + 2), fa.ERR_ALIGN),
                     (dict(ref=t[8:]), fa.ERR_ARG), (dict(r=65), fa.ERR_ARG), (dict(plan_bytes=48), fa.ERR_ARG)):
        args = dict(plan=t, f=t, r=1, cnt=16, dst=t, plan_bytes=32)
        args.update(kw)
        with pytest.raises(fa.FaError) as ei:
            fa.lowrank_expand_device(**args)
        assert ei.value.code == code, kw
