"""GPU: fa_topk_expand_device and fa_topk_encode_device (fa.h "Top-k receipts") against tests/topk_ref.py, every bit
(NaN as NaN).

Both kernels work in tiles of T = 4096 elements, 16 consecutive elements per lane, laid over the launch so that lanes
start at 16 bytes where the pointers' phases agree.  The sizes sit on both sides of a tile and span several; the
pointers are aligned, off 16 bytes in agreement (the first tile is padded), and in disagreement (one element at a
time).  The slot lies between guard bands (tests/guarded.py) that must survive.
"""
import numpy as np
import pytest

import guarded as G
import topk_ref as K
from test_mx8_gpu import ITEM, NP_DT, PAIR_IDS, PAIRS, SPECIALS, at_phase, fa_dt

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
T = 4096


def phase_sets(slot_kind, ref_kind):
    """(slot, reference) element phases: aligned; one element off with the reference in agreement; in disagreement."""
    if ref_kind is None:
        return [(0, 0), (1, 0)]
    head = 16 // ITEM[slot_kind] - 1  # the slot one element off: this many elements to its 16-byte boundary
    agree = -head % (16 // ITEM[ref_kind])
    return [(0, 0), (1, agree), (1, (agree + 1) % (16 // ITEM[ref_kind]))]


def index_sets(n, rng):
    """Local indices: random at k in {0, 1, n / 8, n}; all in one tile; exactly the tile edges; first and last."""
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in (0, 1, max(1, n // 8), n)]
    lo = T if n > T else 0
    tile = np.arange(lo, min(n, lo + T))
    sets.append(np.sort(rng.choice(tile, max(1, tile.size // 3), replace=False)))
    sets.append(np.asarray([i for i in (T - 1, T, 2 * T - 1, 2 * T) if i < n], np.int64))
    sets.append(np.unique([0, n - 1]))
    return sets


@pytest.mark.parametrize("idx0", [0, 33])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_expansion(fa, torch_gpu, pair, idx0):
    slot_kind, ref_kind = pair
    rng = np.random.default_rng(idx0 + 1)
    below = np.asarray([0, idx0 - 1] if idx0 else [], np.int64)
    for n in (1, 17, T - 1, T, T + 1, 3 * T + 5):
        g = K.round_out(rng.uniform(-1, 1, n).astype(F32), ref_kind) if ref_kind else None
        for local in index_sets(n, rng):
            idx = np.concatenate([below, idx0 + local, [idx0 + n, idx0 + n + 5]]).astype(U32)  # two ends to ignore
            val = rng.standard_normal(idx.size).astype(F32)
            want = K.expand(idx, val, n, idx0, slot_kind, g, ref_kind)
            i_v, v_v = at_phase(torch_gpu, idx, 0)[1], at_phase(torch_gpu, val, 0)[1]
            for dp, rp in phase_sets(slot_kind, ref_kind):
                r_v = at_phase(torch_gpu, g, rp * ITEM[ref_kind])[1] if ref_kind else None
                snap = G.snapshot(r_v) if ref_kind else None
                buf = G.GuardedBuf(torch_gpu, n * ITEM[slot_kind], dp * ITEM[slot_kind])
                fa.topk_expand_device(i_v, v_v, idx.size, n, buf.ptr, fa_dt(fa, slot_kind), ref=r_v,
                                      ref_dtype=fa_dt(fa, ref_kind), idx0=idx0)
                torch_gpu.cuda.synchronize()
                what = "%s n %d idx0 %d k %d phases dst%d ref%d" % (PAIR_IDS[PAIRS.index(pair)], n, idx0, local.size, dp, rp)
                K.assert_bits(buf.payload().cpu().numpy().view(NP_DT[slot_kind]).copy(), want, what)
                buf.check(what)
                if ref_kind:
                    G.assert_unchanged(r_v, snap, what)


@pytest.mark.parametrize("pair", [p for p in PAIRS if p[1]], ids=[i for p, i in zip(PAIRS, PAIR_IDS) if p[1]])
def test_expansion_keeps_ieee_edges_under_a_zero_delta(fa, torch_gpu, pair):
    """References -0, inf, NaN, the subnormals: absent elements take the same add, so -0 + +0 is +0."""
    slot_kind, ref_kind = pair
    g = np.tile(SPECIALS[ref_kind], 3)
    idx, val = np.asarray([2], U32), np.asarray([1.5], F32)
    want = K.expand(idx, val, g.size, 0, slot_kind, g, ref_kind)
    assert np.signbit(K.widen(g[1:2], ref_kind))[0] and not want[1:2].view(np.uint8).any()
    buf = G.GuardedBuf(torch_gpu, g.size * ITEM[slot_kind], 0)
    fa.topk_expand_device(at_phase(torch_gpu, idx, 0)[1], at_phase(torch_gpu, val, 0)[1], 1, g.size, buf.ptr,
                          fa_dt(fa, slot_kind), ref=at_phase(torch_gpu, g, 0)[1], ref_dtype=fa_dt(fa, ref_kind))
    torch_gpu.cuda.synchronize()
    K.assert_bits(buf.payload().cpu().numpy().view(NP_DT[slot_kind]).copy(), want, PAIR_IDS[PAIRS.index(pair)])
    buf.check()


def select_once(fa, torch, new, sent, kind, k, out_mode, phase=0):
    """fa.topk_encode_device at element phase `phase` of new / sent (sent one more if phase > 1): (idx, val, g' or None)."""
    n, es = new.size, ITEM[kind]
    kp = min(k, n)
    new_v = at_phase(torch, new, phase * es)[1]
    sent_v = at_phase(torch, sent, (phase + (phase > 1)) * es)[1]
    idx_b, val_b = G.GuardedBuf(torch, max(kp, 1) * 4, 0), G.GuardedBuf(torch, max(kp, 1) * 4, 0)
    out_b = G.GuardedBuf(torch, n * es, phase * es) if out_mode == "apart" else None
    work = torch.full((fa.topk_encode_workspace(n),), 0xA5, dtype=torch.uint8, device="cuda")  # not initialised
    out = {"none": None, "apart": out_b.ptr if out_b else None, "sent": sent_v}[out_mode]
    fa.topk_encode_device(new_v, sent_v, n, k, idx_b.ptr, val_b.ptr, work, out=out, dtype=fa_dt(fa, kind))
    torch.cuda.synchronize()
    for b in (idx_b, val_b, out_b):
        if b is not None:
            b.check("k %d n %d" % (k, n))
    gp = {"none": None, "apart": out_b.payload() if out_b else None, "sent": sent_v}[out_mode]
    return (idx_b.payload().cpu().numpy().view(U32)[:kp].copy(), val_b.payload().cpu().numpy().view(F32)[:kp].copy(),
            None if gp is None else gp.cpu().numpy().view(NP_DT[kind]).copy())


@pytest.mark.parametrize("pattern", K.PATTERNS)
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_selection(fa, torch_gpu, kind, pattern):
    """Every output against the reference.  The tie patterns are taken against sent = +0, so that the deltas are the
    pattern itself; the random one against a random model.  d_out is absent, apart and `sent` itself in turn."""
    step = 0
    for n in (1, 33, T - 1, T + 1, 3 * T + 5):
        new = K.round_out(K.deltas(pattern, n, n), kind)
        sent = K.round_out(K.deltas("random", n, n + 1) if pattern == "random" else np.zeros(n, F32), kind)
        for k in (0, 1, n // 2, n - 1, n, n + 7):
            out_mode = ("none", "apart", "sent")[step % 3]
            step += 1
            what = "%s %s n %d k %d out %s" % (kind, pattern, n, k, out_mode)
            idx, val, gp = select_once(fa, torch_gpu, new, sent, kind, k, out_mode)
            want_idx, want_val, want_gp = K.encode(new, sent, kind, k)
            assert np.array_equal(idx, want_idx), what
            K.assert_bits(val, want_val, what)
            if gp is not None:
                K.assert_bits(gp, want_gp, what)


@pytest.mark.parametrize("phase", [0, 1, 2], ids=["aligned", "agreeing", "mixed"])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_selection_at_pointer_phases_and_the_round_trip(fa, torch_gpu, kind, phase):
    """new, sent and d_out one element off 16 bytes (a padded first tile) and in disagreement (the element form); then
    the expansion of the selected entries against `sent` is g'."""
    n, k = 3 * T + 5, T + 3
    new, sent = (K.round_out(K.deltas("random", n, s), kind) for s in (1, 2))
    idx, val, gp = select_once(fa, torch_gpu, new, sent, kind, k, "apart", phase)
    want_idx, want_val, want_gp = K.encode(new, sent, kind, k)
    assert np.array_equal(idx, want_idx)
    K.assert_bits(val, want_val, "val")
    K.assert_bits(gp, want_gp, "g'")
    buf = G.GuardedBuf(torch_gpu, n * ITEM[kind], 0)
    fa.topk_expand_device(at_phase(torch_gpu, idx, 0)[1], at_phase(torch_gpu, val, 0)[1], idx.size, n, buf.ptr,
                          fa_dt(fa, kind), ref=at_phase(torch_gpu, sent, 0)[1], ref_dtype=fa_dt(fa, kind))
    torch_gpu.cuda.synchronize()
    K.assert_bits(buf.payload().cpu().numpy().view(NP_DT[kind]).copy(), gp, "round trip")


def test_probe_and_refusals_on_the_device(fa, torch_gpu):
    t = torch_gpu.zeros(64, dtype=torch_gpu.float32, device="cuda")
    fa.topk_expand_device(t, t, 0, 0, t)  # n == 0
    fa.topk_encode_device(t, t, 0, 4, t, t, t)
    with pytest.raises(fa.FaError) as ei:
        fa.topk_expand_device(t, t, 1, 4, t.data_ptr() + 2, fa.F32)
    assert ei.value.code == fa.ERR_ALIGN
    with pytest.raises(fa.FaError) as ei:
        fa.topk_encode_device(t.data_ptr() + 2, t, 4, 1, t, t, t)
    assert ei.value.code == fa.ERR_ALIGN
    with fa.Aggregator(1) as agg:
        for call in (lambda: fa.topk_expand_device(t, t, 1, 4, t, gpu=1, ctx=agg),
                     lambda: fa.topk_encode_device(t, t, 4, 1, t, t, t, gpu=1, ctx=agg)):
            with pytest.raises(fa.FaError) as ei:
                call()
            assert ei.value.code == fa.ERR_ARG and "gpu" in str(ei.value)
