"""GPU: fa_sparse_sum_device (fa.h "Sparse-sum stage", rules 1-2) against tests/sparse_ref.py, every bit (NaN as NaN).  The
output and the workspace lie between guard bands (tests/guarded.py) that must survive.

E: the kernel's tile sizes (fa.SPARSE_TILES = 2048, 8192), G = fa.SPARSE_GROUP = 4 its prefetch depth.  The host takes the
big tile where 2048 sum k < D n; a test reaches a tile through the density of its receipts (k_c up to n / 8: the small one,
up to n / 4096: the big one) and asserts the form through fa.sparse_sum_form, or forces it (tile=) where the issue's shape
fixes the density.  The covering set, stated openly:
  CLIENTS  D in {1, 2, 3, G - 1, G, G + 1, 127, 128} at n = 3 E + E / 2 + 1 of each tile; random k_c, client 1 with none;
           bucket offset 77, so entries fall outside the range on both sides;
  SIZES    n in {1, 15, 16, 17, E - 1, E, E + 1, 3 E + E / 2 + 1} for each E at D = 8, both tiles forced at every n; entries
           planted on the first and last element of every tile (of the unpadded and of the padded lay-out) and of the
           launch; (g, output) at element offsets (0, 0), (1, 1) and (0, 1).  By the one rule of fa_split.h a common
           offset of 1 is a head and stays the vector form; it is the disagreeing pair (0, 1) that forces the element form;
  ORDER    D = 16 clients with one index set, values times 2^(8 c mod 40) under mixed-sign weights; (1e8, 1, -1e8) from
           three clients to one element;
  DENSITY  k_c = n for all clients at n = E + 17 (every lane loop runs more than once); one entry in the whole launch;
  PAIRS    the seven dtype pairs and 16-bit absolute mode at two n, g with an fp16 subnormal and 65504;
  INPUTS   NaN, inf and -0 in val and in g; weights 0, negative and inf; idx and val 4 and 8 bytes past a 16-byte boundary.
"""
import numpy as np
import pytest

import guarded as G
import sparse_ref as S
from test_mx8_gpu import ITEM, NP_DT, at_phase, fa_dt

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
TILES = (2048, 8192)
DS = [1, 2, 3, 4, 5, 127, 128]  # G - 1, G, G + 1 = 3, 4, 5
PAIRS = [("f32", "f32"), ("f32", "bf16"), ("f32", "f16"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32"),
         (None, "bf16"), (None, "f16")]  # (reference, output); None: absolute mode


def big_n(E):
    return 3 * E + E // 2 + 1


def run_sum(fa, torch, idx, val, w, n, idx0=0, g=None, ref_kind="f32", out_kind="f32", offs=(0, 0), phase=0, tile=None):
    """One call on the device against the reference; returns the form the host would take by itself."""
    want = S.sparse_sum(idx, val, w, n, idx0, None if g is None else S.widen(g, ref_kind))
    keep = [(at_phase(torch, i, phase), at_phase(torch, v, phase)) for i, v in zip(idx, val)]
    r_v = at_phase(torch, g, offs[0] * ITEM[ref_kind])[1] if g is not None else None
    out = G.GuardedBuf(torch, n * ITEM[out_kind], offs[1] * ITEM[out_kind])
    work = G.GuardedBuf(torch, fa.sparse_sum_workspace(n, len(idx)))
    k = [i.size for i in idx]
    form = fa.sparse_sum_form(n, k, out.ptr, fa_dt(fa, out_kind), r_v, fa_dt(fa, ref_kind))
    fa.sparse_sum_device([a[1] for a, _ in keep], [b[1] for _, b in keep], k, n, out.ptr, work.ptr, fa_dt(fa, out_kind), w,
                         r_v, fa_dt(fa, ref_kind), idx0, tile)
    torch.cuda.synchronize()
    what = "D %d n %d idx0 %d %s->%s offs %s phase %d form %d tile %s" % (len(idx), n, idx0, ref_kind, out_kind, offs, phase, form, tile)
    S.assert_bits(out.payload().cpu().numpy().view(NP_DT[out_kind]), S.round_out(want, out_kind), what)
    out.check(what)
    work.check(what)
    assert bool(form & fa.SPARSE_BIG_TILE) == (2048 * sum(k) < len(idx) * n), what
    return form


def reference(n, kind, seed):
    return S.round_out(np.random.default_rng(seed).standard_normal(n).astype(F32), kind)


def weights(D, seed):
    return (np.random.default_rng(seed).standard_normal(D) * np.where(np.arange(D) % 3, 1.0, -1.0)).astype(F32)


@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("D", DS)
def test_clients(fa, torch_gpu, D, big):
    n, idx0 = big_n(TILES[big]), 77
    idx, val = S.receipts(D, idx0 + n + 99, n // (4096 if big else 8), 10 * D + big, empty={1})
    form = run_sum(fa, torch_gpu, idx, val, weights(D, D), n, idx0, reference(n, "f32", D))
    assert form == fa.SPARSE_VECTOR | (fa.SPARSE_BIG_TILE if big else 0)


@pytest.mark.parametrize("n", sorted({1, 15, 16, 17} | {e + d for e in TILES for d in (-1, 0, 1)} | {big_n(e) for e in TILES}))
def test_sizes(fa, torch_gpu, n):
    D, idx0 = 8, 77
    idx, val = S.receipts(D, idx0 + n + 99, max(1, n // 8), n)
    edges = {0, n - 1} | {t * e + d for e in TILES for t in range(n // e + 2) for d in (-14, -13, -1, 0)}
    idx, val = S.with_entries(idx, val, [idx0 + i for i in edges if 0 <= i < n] + [idx0 - 1, idx0 + n], n)
    w, g = weights(D, n), reference(n, "f32", n)
    for offs, vec in (((0, 0), True), ((1, 1), True), ((0, 1), False)):
        for tile in (0, 1):
            form = run_sum(fa, torch_gpu, idx, val, w, n, idx0, g, offs=offs, tile=tile)
            if n > 17:  # below that no lane lies inside the launch, and the bit says nothing
                assert bool(form & fa.SPARSE_VECTOR) == vec
    run_sum(fa, torch_gpu, idx, val, w, n, idx0, None, offs=(0, 1))  # absolute mode: the output alone leads, at any phase


def test_order(fa, torch_gpu):
    D, n = 16, 2048 + 300
    rng = np.random.default_rng(5)
    at = np.sort(rng.choice(n, n // 4, replace=False)).astype(U32)
    val = [(rng.standard_normal(at.size) * 2.0 ** (8 * c % 40)).astype(F32) for c in range(D)]
    for tile in (0, 1):
        run_sum(fa, torch_gpu, [at] * D, val, weights(D, 3), n, 0, reference(n, "f32", 1), tile=tile)
    one = [np.array([700], U32)] * 3
    vals = [np.array([v], F32) for v in (1e8, 1.0, -1e8)]
    run_sum(fa, torch_gpu, one, vals, np.ones(3, F32), n)
    assert S.sparse_sum(one, vals, np.ones(3, F32), n)[700] == 0.0  # 1e8 + 1 rounds to 1e8: any other order keeps the 1
    assert S.sparse_sum(one[::-1], [vals[2], vals[0], vals[1]], np.ones(3, F32), n)[700] == 1.0


@pytest.mark.parametrize("big", [0, 1])
def test_density(fa, torch_gpu, big):
    D, n = 6, TILES[big] + 17
    rng = np.random.default_rng(big)
    full = [np.arange(n, dtype=U32)] * D
    run_sum(fa, torch_gpu, full, [rng.standard_normal(n).astype(F32) for _ in range(D)], weights(D, 9), n, 0,
            reference(n, "f32", 2), tile=big)
    lone = [np.zeros(0, U32)] * (D - 1) + [np.array([n - 1], U32)]
    form = run_sum(fa, torch_gpu, lone, [np.zeros(0, F32)] * (D - 1) + [np.array([3.0], F32)], weights(D, 9), n, 0,
                   reference(n, "f32", 2), tile=big)
    assert form & fa.SPARSE_BIG_TILE


@pytest.mark.parametrize("pair", PAIRS, ids=["%s->%s" % (r or "abs", o) for r, o in PAIRS])
def test_dtype_pairs(fa, torch_gpu, pair):
    ref_kind, out_kind = pair
    for n in (129, 2048 + 257):
        idx, val = S.receipts(5, n, n // 4, n)
        val = [(v * F32(6e-5)).astype(F32) for v in val]
        g = reference(n, ref_kind, n) if ref_kind else None
        if g is not None and ref_kind != "bf16":
            g[:3] = [6e-8, 65504.0, -6e-5]  # an fp16 subnormal, the largest fp16, a value whose sum is subnormal
        for offs in ((0, 0), (1, 1), (0, 1)):
            run_sum(fa, torch_gpu, idx, val, weights(5, n), n, 0, g, ref_kind or out_kind, out_kind, offs)


def test_inputs(fa, torch_gpu):
    n, D = 2048 + 300, 6
    idx, val = S.receipts(D, n, n // 4, 1)
    for v in val:
        v[::5] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45], F32), v[::5].size)
    g = reference(n, "f32", 1)
    g[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], F32), g[::7].size)
    w = np.array([0.0, -1.0, np.inf, 1e-30, -0.0, 2.0], F32)
    for phase in (0, 4, 8):  # a range piece's phases of idx and val
        run_sum(fa, torch_gpu, idx, val, w, n, 0, g, phase=phase)
    run_sum(fa, torch_gpu, idx, val, w, n, 0, None)
