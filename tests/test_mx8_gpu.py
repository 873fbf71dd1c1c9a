"""GPU: fa_mx8_expand_device (fa.h "MX8 receipts", decode rule 3) against tests/mx8_ref.py, every bit (NaN as NaN).

Sizes around the vector (16 elements) and the block (32), several workgroups and a size at which the element form
strides; bucket offsets that put a vector across two blocks; every (slot, reference) dtype pair and absolute mode;
every byte phase of q and e and every element phase of the reference and the slot within 16 bytes, the mixed ones
that force the element form included; all 256 codes against the scale edges and IEEE edge references; 16-bit sums
that round to inf and to a subnormal.  The slot lies between guard bands (tests/guarded.py) that must survive.
"""
import numpy as np
import pytest

import guarded as G
import mx8_ref as M

pytestmark = pytest.mark.gpu

F16, F32, I8, U8, U16, U32 = np.float16, np.float32, np.int8, np.uint8, np.uint16, np.uint32
NS = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4099, 65537 + 13]
PAIRS = [("f32", "f32"), ("f32", "bf16"), ("f32", "f16"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"),
         ("f16", "f32"), ("f32", None), ("bf16", None), ("f16", None)]  # (slot, reference); None: absolute mode
PAIR_IDS = ["%s<-%s" % (s, r or "abs") for s, r in PAIRS]
ITEM = {"f32": 4, "bf16": 2, "f16": 2}
NP_DT = {"f32": F32, "bf16": U16, "f16": F16}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "bf16": fa.BF16, "f16": fa.F16, None: fa.F32}[kind]


def at_phase(torch, host, phase):
    """`host` (any numpy array) on the device at an address that is `phase` modulo 16: (keep-alive, view)."""
    raw = np.ascontiguousarray(host).view(U8).reshape(-1)
    whole = torch.empty(raw.size + 32, dtype=torch.uint8, device="cuda")
    off = (phase - whole.data_ptr()) % 16
    view = whole[off:off + raw.size]
    view.copy_(torch.from_numpy(np.array(raw)))
    assert view.data_ptr() % 16 == phase % 16
    return whole, view


def make_inputs(n, idx0, ref_kind, seed):
    """(q, e as the bytes of blocks idx0 >> 5 .., g of ref_kind or None): deltas of the references' size."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-128, 128, n).astype(I8)
    e = rng.integers(118, 134, ((idx0 + n - 1) >> 5) - (idx0 >> 5) + 1).astype(U8)
    g = None
    if ref_kind is not None:
        g = M.round_out(rng.uniform(-1, 1, n).astype(F32), ref_kind)
    return q, e, g


def expand_once(fa, torch, q_v, e_v, n, idx0, slot_kind, buf, ref_v, ref_kind):
    fa.mx8_expand_device(q_v, e_v, n, buf.ptr, fa_dt(fa, slot_kind), ref=ref_v, ref_dtype=fa_dt(fa, ref_kind), idx0=idx0)
    torch.cuda.synchronize()
    return buf.payload().cpu().numpy().view(NP_DT[slot_kind]).copy()


# ------------------------------------------------------------------ sizes and bucket offsets

@pytest.mark.parametrize("idx0", M.IDX0S)
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_sizes_and_offsets(fa, torch_gpu, pair, idx0):
    """Every size at 16-byte aligned pointers (the vector form with its head-less split) and at one mixed set of
    phases (the element form)."""
    slot_kind, ref_kind = pair
    for n in NS:
        q, e, g = make_inputs(n, idx0, ref_kind, n * 131 + idx0)
        want = M.expand(q, e, idx0, slot_kind, g, ref_kind)
        for qp, dp, rp in ((0, 0, 0), (3, 1, 2)):
            _, q_v = at_phase(torch_gpu, q, qp)
            _, e_v = at_phase(torch_gpu, e, (qp * 7 + 5) % 16)
            r_keep, r_v = at_phase(torch_gpu, g, rp * ITEM[ref_kind]) if g is not None else (None, None)
            snap = G.snapshot(r_v) if g is not None else None
            buf = G.GuardedBuf(torch_gpu, n * ITEM[slot_kind], dp * ITEM[slot_kind])
            got = expand_once(fa, torch_gpu, q_v, e_v, n, idx0, slot_kind, buf, r_v, ref_kind)
            what = "%s n %d idx0 %d phases q%d dst%d ref%d" % (PAIR_IDS[PAIRS.index(pair)], n, idx0, qp, dp, rp)
            M.assert_bits(got, want, what)
            buf.check(what)
            if g is not None:
                G.assert_unchanged(r_v, snap, what)


def test_element_form_strides(fa, torch_gpu):
    """More elements than one trip of the element form's capped grid (2^14 workgroups of 256): it strides."""
    n, idx0 = (1 << 22) + 77, 33
    q, e, g = make_inputs(n, idx0, "f32", 5)
    want = M.expand(q, e, idx0, "f32", g, "f32")
    _, q_v = at_phase(torch_gpu, q, 1)
    _, e_v = at_phase(torch_gpu, e, 9)
    _, r_v = at_phase(torch_gpu, g, 8)
    buf = G.GuardedBuf(torch_gpu, n * 4, 4)
    got = expand_once(fa, torch_gpu, q_v, e_v, n, idx0, "f32", buf, r_v, "f32")
    M.assert_bits(got, want, "n %d" % n)
    buf.check("n %d" % n)


# ------------------------------------------------------------------ pointer phases

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_every_pointer_phase(fa, torch_gpu, pair):
    """q at each of 16 byte phases x the slot at each element phase within 16 bytes x the reference at each of its
    own; e walks through its 16 byte phases on the way.  Where the three agree on a head the vector form runs
    (head, vectors, tail), everywhere else the element form: the bits are the same."""
    slot_kind, ref_kind = pair
    idx0 = 33
    seen_vec = seen_elem = 0
    for n in (17, 257):
        q, e, g = make_inputs(n, idx0, ref_kind, n)
        want = M.expand(q, e, idx0, slot_kind, g, ref_kind)
        q_at = [at_phase(torch_gpu, q, p) for p in range(16)]
        e_at = [at_phase(torch_gpu, e, p) for p in range(16)]
        r_phases = range(16 // ITEM[ref_kind]) if g is not None else [0]
        r_at = [at_phase(torch_gpu, g, p * ITEM[ref_kind]) for p in r_phases] if g is not None else [(None, None)]
        step = 0
        for dp in range(16 // ITEM[slot_kind]):
            buf = G.GuardedBuf(torch_gpu, n * ITEM[slot_kind], dp * ITEM[slot_kind])
            for qp in range(16):
                for rp in r_phases:
                    got = expand_once(fa, torch_gpu, q_at[qp][1], e_at[step % 16][1], n, idx0, slot_kind, buf,
                                      r_at[rp][1], ref_kind)
                    step += 1
                    what = "%s n %d phases q%d dst%d ref%d" % (PAIR_IDS[PAIRS.index(pair)], n, qp, dp, rp)
                    M.assert_bits(got, want, what)
                    # the rule of fa_split.h, restated: a common head h = -q mod 16 that aligns the other two
                    h = (16 - qp) % 16
                    vec = (dp + h) * ITEM[slot_kind] % 16 == 0 and (g is None or (rp + h) * ITEM[ref_kind] % 16 == 0)
                    seen_vec += vec and n - h >= 16
                    seen_elem += not vec
            buf.check("%s n %d dst phase %d" % (PAIR_IDS[PAIRS.index(pair)], n, dp))
    assert seen_vec > 0 and seen_elem > 0


# ------------------------------------------------------------------ codes, scales, edge references

SPECIALS = {
    "f32": np.asarray([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000,
                       0xFF800000, 0x7FC00000, 0x3F800000, 0xBFC00000], U32).view(F32),
    "bf16": np.asarray([0x0000, 0x8000, 0x0001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xBFC0],
                       U16),
    "f16": np.asarray([0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x3C00, 0xBE00],
                      U16).view(F16),
}


@pytest.mark.parametrize("phases", [(0, 0, 0), (5, 1, 3)], ids=["vector", "element"])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_codes_scale_edges_and_special_references(fa, torch_gpu, pair, phases):
    """All 256 codes x the scale edges (subnormal scales, 2^0, the -2^128 -> -inf pair, NaN at 255) x references +-0,
    the smallest and largest subnormal and normal, +-inf and NaN: one launch, block after block."""
    slot_kind, ref_kind = pair
    codes = np.arange(-128, 128).astype(I8)
    one = np.tile(codes, len(M.E_EDGES))                           # 11 x 256 elements = 88 blocks
    e_one = np.repeat(np.asarray(M.E_EDGES, U8), 256 // 32)
    specials = SPECIALS[ref_kind] if ref_kind is not None else np.zeros(1, F32)
    q, e = np.tile(one, specials.size), np.tile(e_one, specials.size)
    g = np.repeat(specials, one.size) if ref_kind is not None else None
    n = q.size
    want = M.expand(q, e, 0, slot_kind, g, ref_kind)
    if ref_kind is not None:  # what the table is there for
        w32 = M.widen(want, slot_kind)
        assert np.isnan(w32).any() and np.isinf(w32).any() and (w32 == 0).any()
        with np.errstate(all="ignore"):
            assert (M.widen(g, ref_kind) + M.decode(q, e) == 0).any()
    qp, dp, rp = phases
    _, q_v = at_phase(torch_gpu, q, qp)
    _, e_v = at_phase(torch_gpu, e, 11)
    _, r_v = at_phase(torch_gpu, g, rp * ITEM[ref_kind]) if g is not None else (None, None)
    buf = G.GuardedBuf(torch_gpu, n * ITEM[slot_kind], dp * ITEM[slot_kind])
    got = expand_once(fa, torch_gpu, q_v, e_v, n, 0, slot_kind, buf, r_v, ref_kind)
    M.assert_bits(got, want, PAIR_IDS[PAIRS.index(pair)])
    buf.check(PAIR_IDS[PAIRS.index(pair)])
    if ref_kind is not None:
        # -0 + +0 is +0: code 0 against the -0 reference
        i = one.size + 128
        assert q[i] == 0 and np.signbit(M.widen(g[i:i + 1], ref_kind))[0]
        assert got[i:i + 1].view(U8).any() == 0, "-0 + +0 must be +0"


# (slot, reference value as fp32, q, E, what the slot must hold): one block each
ROUNDING = [
    ("f16", 65504.0, 1, 138, np.inf),            # 65504 + 32 = 65536: beyond the largest fp16, to inf
    ("f16", 65504.0, 1, 137, np.inf),            # 65504 + 16: the tie goes to the even side, which is 2^16: inf
    ("f16", 65504.0, 1, 136, 65504.0),           # 65504 + 8: back to the largest fp16
    ("f16", 0.0, 5, 107, 2.0 ** -24),            # 1.25 x 2^-24: to the smallest fp16 subnormal
    ("f16", 0.0, 3, 108, 2.0 ** -23),            # 1.5 x 2^-24: the tie goes to the even 2 x 2^-24
    ("f16", 2.0 ** -14, -1, 109, 1023 * 2.0 ** -24),  # the smallest normal less one step: the largest subnormal
    ("bf16", float(np.asarray([0x7F7F0000], U32).view(F32)[0]), 1, 252, np.inf),  # max bf16 + half a step: to inf
    ("bf16", 0.0, 5, 0, 5 * 2.0 ** -133),        # a bf16 subnormal, exact
    ("bf16", 0.0, 5, 1, 10 * 2.0 ** -133),
    ("bf16", 2.0 ** -140, 3, 0, 3 * 2.0 ** -133),  # 3 x 2^-133 + 2^-140 rounds back to the subnormal 3 x 2^-133
    ("bf16", 2.0 ** -126, -1, 0, 127 * 2.0 ** -133),  # the largest bf16 subnormal
]


def test_sixteen_bit_slots_round_to_inf_and_to_subnormals(fa, torch_gpu):
    for slot_kind in ("f16", "bf16"):
        rows = [r for r in ROUNDING if r[0] == slot_kind]
        n = 32 * len(rows)
        q, e, g = np.zeros(n, I8), np.zeros(len(rows), U8), np.zeros(n, F32)
        for b, (_, gv, qv, E, _) in enumerate(rows):
            q[32 * b], e[b], g[32 * b] = qv, E, gv
        want = M.expand(q, e, 0, slot_kind, g, "f32")
        for b, row in enumerate(rows):  # the reference against the values written down above
            assert M.widen(want[32 * b:32 * b + 1], slot_kind)[0] == F32(row[4]), row
        w32 = M.widen(want, slot_kind)
        tiny = 2.0 ** -14 if slot_kind == "f16" else 2.0 ** -126
        assert np.isinf(w32).any() and ((w32 != 0) & (np.abs(w32) < tiny)).any()
        for qp in (0, 9):
            _, q_v = at_phase(torch_gpu, q, qp)
            _, e_v = at_phase(torch_gpu, e, 0)
            _, r_v = at_phase(torch_gpu, g, 0)
            buf = G.GuardedBuf(torch_gpu, n * 2, 0)
            got = expand_once(fa, torch_gpu, q_v, e_v, n, 0, slot_kind, buf, r_v, "f32")
            M.assert_bits(got, want, "%s q phase %d" % (slot_kind, qp))
            buf.check(slot_kind)


def test_probe_and_refusals_on_the_device(fa, torch_gpu):
    t = torch_gpu.zeros(64, dtype=torch_gpu.float32, device="cuda")
    fa.mx8_expand_device(t, t, 0, t)  # n == 0
    with pytest.raises(fa.FaError) as ei:
        fa.mx8_expand_device(t, t, 4, t.data_ptr() + 2, fa.F32)
    assert ei.value.code == fa.ERR_ALIGN
    with fa.Aggregator(1) as agg:
        with pytest.raises(fa.FaError) as ei:
            fa.mx8_expand_device(t, t, 4, t, gpu=1, ctx=agg)
        assert ei.value.code == fa.ERR_ARG and "gpu" in str(ei.value)
