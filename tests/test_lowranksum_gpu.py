"""GPU: fa_lowrank_sum_device (fa.h "Low-rank-sum stage") against tests/lowranksum_ref.py, on raw pointers between guard bands.

The kernel takes tiles of 64 x 128 (two of the plan's 64 x 64 records), stacks the owners' ranks, each padded to a multiple
of 4, into chunks of 32 columns that alternate between two LDS buffers, and stores runs of 8 laid on the output's 16-byte
grid.  The bucket of lowrank_ref has a matrix on every side of those sizes; the rank vectors are one k-step, whole k-steps,
a stack that crosses a chunk in mid-owner and wraps both buffers (3 + 5 + 1 + 64 + 2 -> 4 + 8 + 4 + 64 + 4 = 84 columns, three
chunks), and nine owners of rank 1, which is three quarters padding.  On lattice data every sum is exact, so every bit must
agree (NaN as NaN).
"""
import functools

import numpy as np
import pytest

import guarded as G
import lowrank_ref as L
import lowranksum_ref as R
from test_lowrank_gpu import MATS, N, RANGES, WIDE
from test_mx8_gpu import ITEM, NP_DT, PAIR_IDS, PAIRS, at_phase, fa_dt
from test_topk_gpu import phase_sets

pytestmark = pytest.mark.gpu

F32 = np.float32
RANKS = [(1,), (4, 4, 4), (3, 5, 1, 64, 2), (1,) * 9]


@functools.lru_cache(maxsize=None)
def round_of(ranks):
    """(receipts, weights from {1/8 .. 8/8}) on the lattice, checked to be exact in any order."""
    fs = [L.lattice(MATS, N, r, 100 + 7 * c + r) for c, r in enumerate(ranks)]
    w = ((np.arange(len(ranks)) * 3) % 8 + 1).astype(F32) / 8
    R.assert_exact(fs, ranks, w, MATS, N)
    return fs, w


def run_kernel(fa, torch, fs, ranks, w, idx0, cnt, out_kind, g=None, ref_kind=None, dp=0, rp=0, what=""):
    """One launch into a guarded output at element phase dp, the reference at rp: the output's elements."""
    plan = at_phase(torch, fa.lowrank_plan(MATS, N, idx0, cnt), 0)[1]
    f_v = [at_phase(torch, f, 4 * (c % 4))[1] for c, f in enumerate(fs)]
    r_v = at_phase(torch, g, rp * ITEM[ref_kind])[1] if ref_kind else None
    snap = G.snapshot(r_v) if ref_kind else None
    buf = G.GuardedBuf(torch, cnt * ITEM[out_kind], dp * ITEM[out_kind])
    fa.lowrank_sum_device(plan, f_v, ranks, cnt, buf.ptr, fa_dt(fa, out_kind), w, r_v, fa_dt(fa, ref_kind), idx0)
    torch.cuda.synchronize()
    buf.check(what)
    if ref_kind:
        G.assert_unchanged(r_v, snap, what)
    return buf.payload().cpu().numpy().view(NP_DT[out_kind]).copy()


@pytest.mark.parametrize("ranks", RANKS, ids=lambda r: "r" + "-".join(map(str, r)))
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_lattice_rounds_bit_for_bit(fa, torch_gpu, pair, ranks):
    out_kind, ref_kind = pair
    fs, w = round_of(ranks)
    ref = R.round_out(np.random.default_rng(7).uniform(-1, 1, N).astype(F32), ref_kind) if ref_kind else None
    whole = R.lowrank_sum(fs, ranks, w, MATS, N, R.widen(ref, ref_kind) if ref_kind else None)
    for idx0, cnt in RANGES:
        g = ref[idx0:idx0 + cnt] if ref_kind else None
        want = R.round_out(whole[idx0:idx0 + cnt], out_kind)
        for dp, rp in phase_sets(out_kind, ref_kind):
            what = "%s ranks %s [%d, +%d) phases out%d ref%d" % (PAIR_IDS[PAIRS.index(pair)], ranks, idx0, cnt, dp, rp)
            R.assert_bits(run_kernel(fa, torch_gpu, fs, ranks, w, idx0, cnt, out_kind, g, ref_kind, dp, rp, what), want, what)


def test_random_factors_stay_inside_the_rule_s_bound(fa, torch_gpu):
    """|a - S| <= 2^-24 |S| + K 2^-52 sum |p' q| + 2^-150 on every covered element: one rounding of a sum whose adds came in
    any order.  The rest is the chain, every bit."""
    ranks = (64,) * 5
    rng = np.random.default_rng(3)
    fs = [rng.standard_normal(L.length(MATS, N, 64)).astype(F32) for _ in ranks]
    w = rng.uniform(0.5, 1.5, 5).astype(F32)
    S, A = R.sums(fs, ranks, w, MATS, N)
    a = run_kernel(fa, torch_gpu, fs, ranks, w, 0, N, "f32")
    excess = np.abs(a.astype(np.float64) - S) - (2.0 ** -24 * np.abs(S) + sum(ranks) * 2.0 ** -52 * A + 2.0 ** -150)
    assert excess.max() <= 0, "beyond the bound by %g at element %d" % (excess.max(), int(np.argmax(excess)))
    rest = L.rest_mask(MATS, N)
    R.assert_bits(a[rest], S[rest].astype(F32), "rest chain")


def test_non_finite_factors_reach_their_row_and_column_only(fa, torch_gpu):
    ranks = (5, 3, 5)
    fs = [f.copy() for f in round_of(ranks)[0]]
    w = np.array([0.5, 1.0, 0.0], F32)
    L.factors(fs[0], MATS, 5)[0][3][0][3, 0] = np.nan  # owner 0: P[3, 0] of the 65 x 63 matrix
    L.factors(fs[1], MATS, 3)[0][3][1][5, 2] = np.inf  # owner 1: Q[5, 2]
    L.factors(fs[2], MATS, 5)[0][3][0][9, 4] = np.inf  # owner 2, weight 0: 0 * inf is NaN in row 9
    a = run_kernel(fa, torch_gpu, fs, ranks, w, 0, N, "f32")
    bad = np.zeros((65, 63), bool)
    bad[3, :], bad[9, :], bad[:, 5] = True, True, True
    want = np.zeros(N, bool)
    want[WIDE:WIDE + 65 * 63] = bad.reshape(-1)
    assert np.array_equal(~np.isfinite(a), want)
    assert np.isnan(a[WIDE + 9 * 63:WIDE + 10 * 63]).all()
    R.assert_bits(a, R.lowrank_sum(fs, ranks, w, MATS, N), "non-finite factors")


def test_refusals_on_the_device(fa, torch_gpu):
    t = torch_gpu.zeros(64, dtype=torch_gpu.float32, device="cuda")
    for kw, code in ((dict(out=t.data_ptr() + 2), fa.ERR_ALIGN), (dict(f=[t.data_ptr() + 2]), fa.ERR_ALIGN),
                     (dict(ref=t[8:]), fa.ERR_ARG), (dict(r=[65]), fa.ERR_ARG), (dict(plan_bytes=48), fa.ERR_ARG)):
        args = dict(plan=t, f=[t], r=[1], cnt=16, out=t, plan_bytes=32)
        args.update(kw)
        with pytest.raises(fa.FaError) as ei:
            fa.lowrank_sum_device(**args)
        assert ei.value.code == code, kw
