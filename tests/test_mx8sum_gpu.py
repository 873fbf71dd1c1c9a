"""GPU: fa_mx8_sum_device (fa.h "MX8-sum stage") against tests/mx8sum_ref.py, every bit (NaN as NaN), the output between
guard bands.  T = fa.MX8_SUM_TILE, GRP = fa.MX8_SUM_GROUP.  Every block's E is drawn from E_EDGES and a third of the codes
from -128, +-127, +-1, 0 unless a test says otherwise: NaN blocks, -inf and subnormal scales lie in every launch."""
import numpy as np
import pytest

import guarded as G
import mx8sum_ref as M
from test_mx8_gpu import ITEM, NP_DT, at_phase, fa_dt
from test_sparse_gpu import PAIRS, reference, weights  # (reference, output) pairs, None: absolute mode; g; mixed-sign w
from test_mx8sum_cpu import order_case

pytestmark = pytest.mark.gpu

F32 = np.float32
T, GRP = 4096, 4
BIG = 3 * T + T // 2 + 1


def run_sum(fa, torch, q, e, w, idx0=0, g=None, ref_kind="f32", out_kind="f32", offs=(0, 0), qphase=0, ephase=0):
    """One call on the device against the reference; returns the form, checked against the rule restated: the head that
    brings the output to 16 bytes must do so for g and every q and land on a multiple of 16 of the bucket."""
    n = q[0].size
    want = M.mx8_sum(q, e, w, idx0, None if g is None else M.widen(g, ref_kind))
    keep = [(at_phase(torch, a, qphase), at_phase(torch, b, ephase)) for a, b in zip(q, e)]
    r_v = at_phase(torch, g, offs[0] * ITEM[ref_kind])[1] if g is not None else None
    out = G.GuardedBuf(torch, n * ITEM[out_kind], offs[1] * ITEM[out_kind])
    form = fa.mx8_sum_form(n, [a[1] for a, _ in keep], out.ptr, fa_dt(fa, out_kind), r_v, fa_dt(fa, ref_kind), idx0)
    fa.mx8_sum_device([a[1] for a, _ in keep], [b[1] for _, b in keep], n, out.ptr, fa_dt(fa, out_kind), w, r_v,
                      fa_dt(fa, ref_kind), idx0)
    torch.cuda.synchronize()
    what = "D %d n %d idx0 %d %s->%s offs %s phases %d %d form %d" % (len(q), n, idx0, ref_kind, out_kind, offs, qphase, ephase, form)
    M.assert_bits(out.payload().cpu().numpy().view(NP_DT[out_kind]), M.round_out(want, out_kind), what)
    out.check(what)
    lead = -offs[1] % (16 // ITEM[out_kind])
    vec = (idx0 + lead) % 16 == 0 and (qphase + lead) % 16 == 0 and (g is None or (offs[0] + lead) * ITEM[ref_kind] % 16 == 0)
    assert form == (fa.MX8_SUM_VECTOR if vec else 0), what
    return form


@pytest.mark.parametrize("D", [1, 2, GRP - 1, GRP, GRP + 1, 127, 128])
def test_clients(fa, torch_gpu, D):
    q, e = M.receipts(D, BIG, 192, D)
    assert run_sum(fa, torch_gpu, q, e, weights(D, D), 192, reference(BIG, "f32", D)) == fa.MX8_SUM_VECTOR


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, T - 1, T, T + 1, BIG])
def test_sizes(fa, torch_gpu, n):
    D, w, g = 8, weights(8, n), reference(n, "f32", n)
    for idx0 in M.IDX0S:
        q, e = M.receipts(D, n, idx0, n + idx0)
        for offs in ((0, 0), (1, 1), (0, 1)):
            form = run_sum(fa, torch_gpu, q, e, w, idx0, g, offs=offs)
            assert form == (fa.MX8_SUM_VECTOR if offs == (0, 0) and idx0 % 16 == 0 else 0)  # odd idx0, (0, 1): element form
        run_sum(fa, torch_gpu, q, e, w, idx0, None, offs=(0, 1))  # absolute mode
    # a head of 3 elements before the first vector, which starts half a block into the bucket's blocks
    q, e = M.receipts(D, n, 205, n)
    assert run_sum(fa, torch_gpu, q, e, w, 205, g, offs=(1, 1), qphase=13) == fa.MX8_SUM_VECTOR


@pytest.mark.parametrize("qphase", [0, 1, 4])
def test_phases(fa, torch_gpu, qphase):
    q, e = M.receipts(6, T + 300, 64, qphase)
    assert run_sum(fa, torch_gpu, q, e, weights(6, 1), 64, reference(T + 300, "f32", 1), qphase=qphase, ephase=3) == (
        0 if qphase else fa.MX8_SUM_VECTOR)


def test_order(fa, torch_gpu):
    for rev in (False, True):
        run_sum(fa, torch_gpu, *order_case(rev))
    D, n = 16, T + 300  # scales 2^(8 c mod 40) apart under mixed-sign weights
    q, _ = M.receipts(D, n, 0, 5)
    e = [np.full((n + 31) // 32, 120 + 8 * c % 40, np.uint8) for c in range(D)]
    run_sum(fa, torch_gpu, q, e, weights(D, 3), 0, reference(n, "f32", 1))


@pytest.mark.parametrize("pair", PAIRS, ids=["%s->%s" % (r or "abs", o) for r, o in PAIRS])
def test_dtype_pairs(fa, torch_gpu, pair):
    ref_kind, out_kind = pair
    for n in (129, T + 257):
        q, e = M.receipts(5, n, 0, n, edges=False)
        e = [(x - 20).astype(np.uint8) for x in e]  # deltas around 2^-26 .. 2^-7: sums that land on fp16 subnormals
        g = reference(n, ref_kind, n) if ref_kind else None
        if g is not None and ref_kind != "bf16":
            g[:3] = [6e-8, 65504.0, -6e-5]  # an fp16 subnormal, the largest fp16, a value whose sum is subnormal
        for offs in ((0, 0), (1, 1), (0, 1)):
            run_sum(fa, torch_gpu, q, e, weights(5, n), 0, g, ref_kind or out_kind, out_kind, offs)


def test_inputs(fa, torch_gpu):
    n = T + 300
    q, e = M.receipts(5, n, 32, 1)
    g = reference(n, "f32", 1)
    g[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], F32), g[::7].size)
    w = np.array([0.0, -1.0, np.inf, 1e-30, -0.0], F32)
    run_sum(fa, torch_gpu, q, e, w, 32, g)
    run_sum(fa, torch_gpu, q, e, w[[0, 1, 3, 4, 1]], 32, g)  # without the inf weight, which leaves only NaN and inf
