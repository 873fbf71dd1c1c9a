"""GPU: fa_rot1_expand_device and fa_rot1_encode_device (fa.h "Rot1 receipts") against tests/rot1_ref.py, every bit
(NaN as NaN).  The ranges start and end inside, at and across block borders of a bucket of n = 3 * 4096 + 5; a single
set bit at position p makes v column p of H_4096, so each index bit that the MFMA layout could mix up has its own case.
The slot lies between guard bands (tests/guarded.py) that must survive."""
import numpy as np
import pytest

import guarded as G
import rot1_ref as R
from test_mx8_gpu import ITEM, NP_DT, PAIR_IDS, PAIRS, SPECIALS, at_phase, fa_dt
from test_topk_gpu import phase_sets

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
B, W = R.B, R.WORDS
N, NB = 3 * B + 5, 4
SEED = 0x9E3779B97F4A7C15
RANGES = [(0, 1), (0, B - 1), (0, B), (0, B + 1), (64, B), (B + 64, 2 * B + 5 - 64)]
COLUMNS = [1 << k for k in range(12)] + [B - 1] + [3, 0x555, 0xAAA]  # a bit position per block of four receipts


def receipts():
    """(name, bits, scale), made once."""
    rng = np.random.default_rng(5)
    rand = lambda k: (F32(0.01) * rng.uniform(0.5, 2, k)).astype(F32)  # noqa: E731
    out = [("random a", rng.integers(0, 1 << 32, NB * W, dtype=np.uint64).astype(U32),
            np.asarray([rand(1)[0], 0.0, -0.0, np.inf], F32)),
           ("random b", rng.integers(0, 1 << 32, NB * W, dtype=np.uint64).astype(U32),
            np.concatenate([np.asarray([np.nan, 1e-42], F32), rand(2)])),
           ("zero bits", np.zeros(NB * W, U32), rand(NB))]
    for k in range(0, len(COLUMNS), NB):
        bits = np.zeros(NB * W, U32)
        for b, p in enumerate(COLUMNS[k:k + NB]):
            bits[b * W + (p >> 5)] = U32(1) << U32(p & 31)
        out.append(("columns %s" % COLUMNS[k:k + NB], bits, rand(NB)))
    return out


RECEIPTS = receipts()


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_expansion(fa, torch_gpu, pair):
    slot_kind, ref_kind = pair
    rng = np.random.default_rng(1)
    g_all = R.round_out(rng.uniform(-1, 1, N).astype(F32), ref_kind) if ref_kind else None
    for name, bits, scale in RECEIPTS:
        for idx0, cnt in RANGES:
            g = g_all[idx0:idx0 + cnt] if ref_kind else None
            bits0, scale0 = bits[(idx0 >> 12) * W:], scale[idx0 >> 12:]
            want = R.expand(bits0, scale0, SEED, idx0, cnt, slot_kind, g, ref_kind)
            b_v, s_v = at_phase(torch_gpu, bits0, 0)[1], at_phase(torch_gpu, scale0, 0)[1]
            for dp, rp in phase_sets(slot_kind, ref_kind):
                r_v = at_phase(torch_gpu, g, rp * ITEM[ref_kind])[1] if ref_kind else None
                snap = G.snapshot(r_v) if ref_kind else None
                buf = G.GuardedBuf(torch_gpu, cnt * ITEM[slot_kind], dp * ITEM[slot_kind])
                fa.rot1_expand_device(b_v, s_v, SEED, cnt, buf.ptr, fa_dt(fa, slot_kind), ref=r_v,
                                      ref_dtype=fa_dt(fa, ref_kind), idx0=idx0)
                torch_gpu.cuda.synchronize()
                what = "%s %s [%d, +%d) phases dst%d ref%d" % (PAIR_IDS[PAIRS.index(pair)], name, idx0, cnt, dp, rp)
                R.assert_bits(buf.payload().cpu().numpy().view(NP_DT[slot_kind]).copy(), want, what)
                buf.check(what)
                if ref_kind:
                    G.assert_unchanged(r_v, snap, what)


@pytest.mark.parametrize("pair", [p for p in PAIRS if p[1]], ids=[i for p, i in zip(PAIRS, PAIR_IDS) if p[1]])
def test_expansion_keeps_ieee_edges_under_a_zero_scale(fa, torch_gpu, pair):
    """References -0, inf, NaN, the subnormals against d = +-0: -0 + +0 must be +0."""
    slot_kind, ref_kind = pair
    g = np.tile(SPECIALS[ref_kind], 40)
    bits, scale = RECEIPTS[0][1], np.zeros(1, F32)
    want = R.expand(bits, scale, SEED, 0, g.size, slot_kind, g, ref_kind)
    g32, d = R.widen(g, ref_kind), R.decode(bits, scale, SEED, 0, g.size)
    hit = np.signbit(g32) & (g32 == 0) & ~np.signbit(d)
    assert hit.any() and not np.signbit(R.widen(want, slot_kind)[hit]).any()
    buf = G.GuardedBuf(torch_gpu, g.size * ITEM[slot_kind], 0)
    fa.rot1_expand_device(at_phase(torch_gpu, bits, 0)[1], at_phase(torch_gpu, scale, 0)[1], SEED, g.size, buf.ptr,
                          fa_dt(fa, slot_kind), ref=at_phase(torch_gpu, g, 0)[1], ref_dtype=fa_dt(fa, ref_kind))
    torch_gpu.cuda.synchronize()
    R.assert_bits(buf.payload().cpu().numpy().view(NP_DT[slot_kind]).copy(), want, PAIR_IDS[PAIRS.index(pair)])
    buf.check()


def models(kind, content, n):
    """(new, sent) of `kind` whose first block's deltas are `content`; Gaussian deltas elsewhere."""
    rng = np.random.default_rng(n)
    sent = rng.uniform(-1, 1, n).astype(F32)
    new = (sent + F32(0.01) * rng.standard_normal(n).astype(F32)).astype(F32)
    m = min(n, B)
    if content == "wide":  # 40 binades, from fp16's subnormals to its top: the fp32 order and the fp64 tree matter
        sent[:m] = 0
        new[:m] = np.ldexp(rng.uniform(1, 2, m) * rng.choice([-1.0, 1.0], m), rng.integers(-25, 15, m)).astype(F32)
    elif content == "equal":  # equal deltas; and a block of deltas +0, whose y are all +-0: only the `< 0` rule
        sent[:m] = 0
        new[:m] = 0.375
        new[B:2 * B] = sent[B:2 * B]
    elif content == "nan":
        new[m // 2] = np.nan
    return R.round_out(new, kind), R.round_out(sent, kind)


@pytest.mark.parametrize("content", ["gaussian", "wide", "equal", "nan"])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_encoder(fa, torch_gpu, kind, content):
    es = ITEM[kind]
    for n in (1, B - 1, B, B + 1, 3 * B + 5):
        new, sent = models(kind, content, n)
        want_bits, want_scale, want_gp = R.encode(new, sent, kind, SEED)
        nb = R.blocks(n)
        for out_mode, phase in (("none", 0), ("sent", 0), ("new", 0), ("apart", 0), ("apart", 1)):
            new_v, sent_v = at_phase(torch_gpu, new, phase * es)[1], at_phase(torch_gpu, sent, phase * es)[1]
            bits_b, scale_b = G.GuardedBuf(torch_gpu, nb * W * 4, 0), G.GuardedBuf(torch_gpu, nb * 4, 0)
            out_b = G.GuardedBuf(torch_gpu, n * es, phase * es) if out_mode == "apart" else None
            out = {"none": None, "apart": out_b.ptr if out_b else None, "sent": sent_v, "new": new_v}[out_mode]
            fa.rot1_encode_device(new_v, sent_v, n, SEED, bits_b.ptr, scale_b.ptr, out=out, dtype=fa_dt(fa, kind))
            torch_gpu.cuda.synchronize()
            what = "%s %s n %d out %s phase %d" % (kind, content, n, out_mode, phase)
            for b in (bits_b, scale_b, out_b):
                if b is not None:
                    b.check(what)
            assert np.array_equal(bits_b.payload().cpu().numpy().view(U32), want_bits), what
            R.assert_bits(scale_b.payload().cpu().numpy().view(F32).copy(), want_scale, what)
            gp = {"none": None, "apart": out_b.payload() if out_b else None, "sent": sent_v, "new": new_v}[out_mode]
            if gp is not None:
                R.assert_bits(gp.cpu().numpy().view(NP_DT[kind]).copy(), want_gp, what)


def test_probe_and_refusals_on_the_device(fa, torch_gpu):
    t = torch_gpu.zeros(B, dtype=torch_gpu.float32, device="cuda")
    fa.rot1_expand_device(t, t, 0, 0, t)  # n == 0
    fa.rot1_encode_device(t, t, 0, 0, t, t)
    with pytest.raises(fa.FaError) as ei:
        fa.rot1_encode_device(t, t, 64, 0, t, t, idx0=64)
    assert ei.value.code == fa.ERR_ARG and "4096" in str(ei.value)
