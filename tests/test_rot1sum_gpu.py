"""GPU: fa_rot1_sum_device (fa.h "Rot1-sum stage") against tests/rot1sum_ref.py, every bit (NaN as NaN), the output between
guard bands.  DEPTH = fa.ROT1_SUM_DEPTH, the owners a lane keeps in flight.  Every third owner has a block with an edge
scale (NaN, +-0, negative, subnormal, 2^100) unless a test says otherwise."""
import numpy as np
import pytest

import guarded as G
import rot1sum_ref as R
from test_mx8_gpu import ITEM, NP_DT, at_phase, fa_dt
from test_sparse_gpu import PAIRS, reference, weights  # (reference, output) pairs, None: absolute mode; g; mixed-sign w

pytestmark = pytest.mark.gpu

F32 = np.float32
B, DEPTH = 4096, 8
BIG = 3 * B + 2049


def run_sum(fa, torch, bits, scale, seed, w, n, idx0=0, g=None, ref_kind="f32", out_kind="f32", offs=(0, 0), ctx=None):
    want = R.rot1_sum(fa, bits, scale, seed, w, n, idx0, None if g is None else R.widen(g, ref_kind))
    keep = [(at_phase(torch, b, 0), at_phase(torch, s, 0)) for b, s in zip(bits, scale)]
    r_v = at_phase(torch, g, offs[0] * ITEM[ref_kind])[1] if g is not None else None
    out = G.GuardedBuf(torch, n * ITEM[out_kind], offs[1] * ITEM[out_kind])
    fa.rot1_sum_device([b[1] for b, _ in keep], [s[1] for _, s in keep], seed, n, out.ptr, fa_dt(fa, out_kind), w, r_v,
                       fa_dt(fa, ref_kind), idx0, ctx=ctx)
    torch.cuda.synchronize()
    what = "D %d n %d idx0 %d %s->%s offs %s" % (len(bits), n, idx0, ref_kind, out_kind, offs)
    R.assert_bits(out.payload().cpu().numpy().view(NP_DT[out_kind]), R.round_out(want, out_kind), what)
    out.check(what)


@pytest.mark.parametrize("D", [1, 2, DEPTH - 1, DEPTH, DEPTH + 1, 127, 128])
def test_clients_one_seed(fa, torch_gpu, D):
    n = 2 * B + 300 if D < 100 else B + 300
    bits, scale, seed = R.receipts(fa, D, n, 192, D)
    run_sum(fa, torch_gpu, bits, scale, seed, weights(D, D), n, 192, reference(n, "f32", D))


@pytest.mark.parametrize("seed", [[1, 2, 3, 4, 5], [7, 9, 7, 9, 11, 7]], ids=["all distinct", "A B A B C A"])
def test_groups(fa, torch_gpu, seed):
    D, n = len(seed), BIG
    bits, scale, _ = R.receipts(fa, D, n, 64, D)
    run_sum(fa, torch_gpu, bits, scale, seed, weights(D, 2), n, 64, reference(n, "f32", 2))


@pytest.mark.parametrize("idx0", [0, 64, 192, 205, B - 16])
@pytest.mark.parametrize("n", [1, 15, 16, 17, B - 1, B, B + 1, BIG])
def test_sizes(fa, torch_gpu, n, idx0):
    D, w, g = 3, weights(3, n), reference(n, "f32", n)
    bits, scale, seed = R.receipts(fa, D, n, idx0, n + idx0, seed=[7, 9, 7])
    for offs in ((0, 0), (1, 1), (0, 1)):
        run_sum(fa, torch_gpu, bits, scale, seed, w, n, idx0, g, offs=offs)
    run_sum(fa, torch_gpu, bits, scale, seed, w, n, idx0, None, offs=(0, 1))  # absolute mode


@pytest.mark.parametrize("pair", PAIRS, ids=["%s->%s" % (r or "abs", o) for r, o in PAIRS])
def test_dtype_pairs(fa, torch_gpu, pair):
    ref_kind, out_kind = pair
    for n in (129, B + 257):
        bits, scale, seed = R.receipts(fa, 5, n, 0, n, edges=False, small=2e-6)  # sums that land on fp16 subnormals
        g = reference(n, ref_kind, n) if ref_kind else None
        if g is not None and ref_kind != "bf16":
            g[:3] = [6e-8, 65504.0, -6e-5]  # an fp16 subnormal, the largest fp16, a value whose sum is subnormal
        for offs in ((0, 0), (1, 1), (0, 1)):
            run_sum(fa, torch_gpu, bits, scale, seed, weights(5, n), n, 0, g, ref_kind or out_kind, out_kind, offs)


def test_inputs(fa, torch_gpu):
    n = B + 300
    bits, scale, seed = R.receipts(fa, 5, n, 64, 1)
    g = reference(n, "f32", 1)
    g[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], F32), g[::7].size)
    w = np.array([0.0, -1.0, np.inf, 1e-30, -0.0], F32)
    run_sum(fa, torch_gpu, bits, scale, seed, w, n, 64, g)
    run_sum(fa, torch_gpu, bits, scale, seed, w[[0, 1, 3, 4, 1]], n, 64, g)  # without the inf weight, which leaves NaN and inf


def test_more_blocks_than_the_grid(fa, torch_gpu):
    """Two workgroups over seven blocks: the kernel strides, and loads the next block's owners under the current one."""
    n = 6 * B + 100
    bits, scale, _ = R.receipts(fa, 10, n, 205, 6)
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=2)
        for seed in (7, [7, 7, 7, 9, 9, 9, 9, 9, 9, 9]):
            run_sum(fa, torch_gpu, bits, scale, seed, weights(10, 6), n, 205, reference(n, "f32", 6), ctx=agg)
