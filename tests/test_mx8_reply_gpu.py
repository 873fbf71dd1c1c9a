"""GPU: fa_mx8_encode_device (fa.h "MX8 replies", rules 3-4 and 6) against tests/mx8_reply_ref.py, every bit of q, e and
g' (NaN as NaN).

Sizes around the vector (16 elements) and the block (32), several workgroups and a size at which the element form
strides; bucket offsets that start a range inside a block; the three dtypes; every byte phase of q and e and every
element phase of the new model, the sent model and the output within 16 bytes, the mixed ones that force the element
form included; the output apart from the inputs, on the sent model and on the new one; blocks whose maximum sits at
both ends of a scale's interval, ties, NaN and inf, 16-bit results that round to inf and land on subnormals; and the
two scale modes around a block that two launches share.  Every buffer lies between guard bands (tests/guarded.py)
that must survive, and the inputs are unchanged where the output is not one of them.
"""
import numpy as np
import pytest

import guarded as G
import mx8_ref as M
import mx8_reply_ref as P

pytestmark = pytest.mark.gpu

F16, F32, F64, I8, U8, U16, U32 = np.float16, np.float32, np.float64, np.int8, np.uint8, np.uint16, np.uint32
NS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 4099, 65537 + 13]
KINDS = ["f32", "bf16", "f16"]
ITEM = {"f32": 4, "bf16": 2, "f16": 2}
NP_DT = {"f32": F32, "bf16": U16, "f16": F16}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "bf16": fa.BF16, "f16": fa.F16}[kind]


def scales_touched(n, idx0):
    return ((idx0 + n - 1) >> 5) - (idx0 >> 5) + 1


def guarded(torch, host, phase_bytes):
    """`host` in a GuardedBuf whose payload starts at `phase_bytes` modulo 16."""
    raw = np.ascontiguousarray(host).view(U8).reshape(-1)
    buf = G.GuardedBuf(torch, raw.size, phase_bytes)
    buf.payload().copy_(torch.from_numpy(np.array(raw)))
    return buf


def read(buf, dtype):
    return buf.payload().cpu().numpy().view(dtype).copy()


def vector_phases(kind, idx0):
    """The phases (q bytes; elements of the new model, the sent one and the output) at which every pointer is on a
    16-byte boundary at the first block boundary of the bucket: the vector form."""
    v = 16 // ITEM[kind]
    return idx0 % 16, idx0 % v, idx0 % v, idx0 % v


def takes_vector(kind, idx0, n, qp, yp, sp, op):
    """The rule of fa_mx8_enc.hip, restated: the head ends at the first block boundary; the vector form runs if every
    pointer is 16-byte aligned there and a whole block follows."""
    h = (32 - idx0 % 32) % 32
    it = ITEM[kind]
    ok = (qp + h) % 16 == 0 and all((p + h) * it % 16 == 0 for p in (yp, sp) + (() if op is None else (op,)))
    return ok and n - h >= 32


def encode_once(fa, torch, y, sent, kind, idx0, phases, ep=0, alias=None, want_out=True, what=""):
    """One fused launch.  phases: (q byte phase, element phases of y, sent, out).  alias: None (out apart), "sent" or
    "new" (out is that input).  Returns (q, e, out or None); checks the guards and that the inputs are unchanged."""
    n = y.size
    qp, yp, sp, op = phases
    it = ITEM[kind]
    yb, sb = guarded(torch, y, yp * it), guarded(torch, sent, sp * it)
    qb = G.GuardedBuf(torch, n, qp)
    eb = G.GuardedBuf(torch, scales_touched(n, idx0), ep)
    ob = G.GuardedBuf(torch, n * it, op * it) if want_out and alias is None else None
    out_ptr = None if not want_out else yb.ptr if alias == "new" else sb.ptr if alias == "sent" else ob.ptr
    fa.mx8_encode_device(yb.ptr, sb.ptr, n, qb.ptr, eb.ptr, out=out_ptr, dtype=fa_dt(fa, kind), idx0=idx0)
    torch.cuda.synchronize()
    for b in (yb, sb, qb, eb) + ((ob,) if ob is not None else ()):
        b.check(what)
    if alias != "new" or not want_out:
        assert np.array_equal(read(yb, U8), np.ascontiguousarray(y).view(U8).reshape(-1)), what + ": the new model changed"
    if alias != "sent" or not want_out:
        assert np.array_equal(read(sb, U8), np.ascontiguousarray(sent).view(U8).reshape(-1)), what + ": the sent model changed"
    out = None
    if want_out:
        out = read(yb if alias == "new" else sb if alias == "sent" else ob, NP_DT[kind])
    return read(qb, I8), read(eb, U8), out


def check(fa, torch, y, sent, kind, idx0, phases, ep=0, alias=None, what=""):
    wq, we, wg = P.reply(y, sent, kind, idx0)
    q, e, out = encode_once(fa, torch, y, sent, kind, idx0, phases, ep, alias, True, what)
    assert np.array_equal(e, we), (what, np.flatnonzero(e != we)[:8], e[:4], we[:4])
    assert np.array_equal(q, wq), (what, np.flatnonzero(q != wq)[:8])
    M.assert_bits(out, wg, what)
    return wq, we, wg


def models(kind, n, seed, step=0.01):
    rng = np.random.default_rng(seed)
    sent = M.round_out(rng.uniform(-1, 1, n).astype(F32), kind)
    # steps of very different sizes from block to block, so the scales differ
    mag = np.repeat(10.0 ** rng.uniform(-4, 0, n // 32 + 2), 32)[:n].astype(F32)
    y = M.round_out((M.widen(sent, kind) + mag * F32(step) * rng.standard_normal(n).astype(F32)).astype(F32), kind)
    return y, sent


# ------------------------------------------------------------------ sizes, bucket offsets, aliasing

@pytest.mark.parametrize("idx0", M.IDX0S)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_and_offsets(fa, torch_gpu, kind, idx0):
    """Every size at the phases that allow the vector form and at one mixed set (the element form); the output apart
    from the inputs, on the sent model and on the new one in turn."""
    seen_vec = 0
    for j, n in enumerate(NS):
        y, sent = models(kind, n, n * 131 + idx0)
        for phases in (vector_phases(kind, idx0), (3, 1, 2, 1)):
            alias = (None, "sent", "new")[(j + phases[0]) % 3]
            what = "%s n %d idx0 %d phases %s alias %s" % (kind, n, idx0, phases, alias)
            check(fa, torch_gpu, y, sent, kind, idx0, phases, (phases[0] * 7 + 5) % 16, alias, what)
            seen_vec += takes_vector(kind, idx0, n, *phases)
    assert seen_vec >= 6


def test_without_an_output(fa, torch_gpu):
    """d_out NULL: the codes alone."""
    for n, idx0, phases in ((257, 0, (0, 0, 0, 0)), (257, 33, (3, 1, 2, 0))):
        y, sent = models("f32", n, 5)
        wq, we, _ = P.reply(y, sent, "f32", idx0)
        q, e, _ = encode_once(fa, torch_gpu, y, sent, "f32", idx0, phases, want_out=False)
        assert np.array_equal(q, wq) and np.array_equal(e, we)


def test_element_form_strides(fa, torch_gpu):
    """More elements than one trip of the element form's capped grid (2^14 workgroups of 256 lanes): it strides."""
    n, idx0 = (1 << 22) + 77, 33
    y, sent = models("f32", n, 7)
    assert not takes_vector("f32", idx0, n, 1, 2, 0, 1)
    check(fa, torch_gpu, y, sent, "f32", idx0, (1, 2, 0, 1), 9, None, "n %d" % n)


# ------------------------------------------------------------------ pointer phases

@pytest.mark.parametrize("kind", KINDS)
def test_every_pointer_phase(fa, torch_gpu, kind):
    """q at each of its 16 byte phases x the new model at each element phase within 16 bytes, with the sent model and
    the output once at the same phase and once at others, so that each of the three visits every phase with every
    phase of q; e walks through its 16 byte phases on the way.  Where all are on a 16-byte boundary at the first block
    boundary the vector form runs (head, blocks, tail), everywhere else the element form: the bits are the same."""
    idx0, v = 33, 16 // ITEM[kind]
    seen_vec = seen_elem = step = 0
    for n in (17, 257):
        y, sent = models(kind, n, n)
        want = P.reply(y, sent, kind, idx0)
        for qp in range(16):
            for yp in range(v):
                for sp, op in ((yp, yp), ((yp + 1) % v, (yp + 3) % v)):
                    what = "%s n %d phases q%d y%d sent%d out%d e%d" % (kind, n, qp, yp, sp, op, step % 16)
                    q, e, out = encode_once(fa, torch_gpu, y, sent, kind, idx0, (qp, yp, sp, op), step % 16, None, True, what)
                    step += 1
                    assert np.array_equal(e, want[1]) and np.array_equal(q, want[0]), what
                    M.assert_bits(out, want[2], what)
                    vec = takes_vector(kind, idx0, n, qp, yp, sp, op)
                    seen_vec += vec
                    seen_elem += not vec
    assert seen_vec > 0 and seen_elem > 0


# ------------------------------------------------------------------ scale edges, ties, non-finite values

def edge_max(E, top):
    """The largest (top) or smallest block maximum whose scale is E: f exactly 127/128 at the top, the next float up at
    the bottom of the scale above."""
    if top:
        return F32(np.ldexp(127.0, E - 133)) if E < 254 else np.finfo(F32).max
    if E == 0:
        return F32(2.0 ** -149)
    return np.nextafter(F32(np.ldexp(127.0, E - 134)), F32(np.inf))


def edge_deltas():
    """(deltas, the E each block must get): per scale edge two blocks, the maximum at the bottom and at the top of the
    scale's interval, the rest of the block fractions of it; then a subnormal maximum, FLT_MAX and a zero block."""
    rng = np.random.default_rng(0xED6E)
    blocks, want = [], []
    for E in [x for x in M.E_EDGES if x != 255]:
        for top in (False, True):
            m = edge_max(E, top)
            with np.errstate(all="ignore"):
                b = (rng.uniform(-1, 1, 32) * F64(m)).astype(F32)
            b[int(rng.integers(32))] = m if top else -m
            blocks.append(b)
            want.append(E)
    sub = np.zeros(32, F32)
    sub[3], sub[20] = F32(2.0 ** -140), F32(-3 * 2.0 ** -149)
    blocks.append(sub)
    want.append(0)
    top = (rng.uniform(-1, 1, 32) * 1e38).astype(F32)
    top[17] = -np.finfo(F32).max
    blocks.append(top)
    want.append(254)
    blocks.append(np.zeros(32, F32))
    want.append(0)
    blocks.append(np.full(32, -0.0, F32))
    want.append(0)
    return np.concatenate(blocks), np.asarray(want, U8)


@pytest.mark.parametrize("form", ["vector", "element"])
def test_scale_edges(fa, torch_gpu, form):
    """f32, the deltas exact: once as y against a zero sent model, once as a zero y against the negated deltas."""
    delta, want_e = edge_deltas()
    phases = (0, 0, 0, 0) if form == "vector" else (5, 1, 3, 2)
    for y, sent in ((delta, np.zeros_like(delta)), (np.zeros_like(delta), -delta)):
        assert np.array_equal(P.deltas(y, sent, "f32").view(U32) & 0x7FFFFFFF, delta.view(U32) & 0x7FFFFFFF)
        _, e, _ = check(fa, torch_gpu, y, sent, "f32", 0, phases, 11, None, "scale edges, %s" % form)
        assert np.array_equal(e, want_e), (e, want_e)  # the table is what it says


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_scale_edges_sixteen_bit(fa, torch_gpu, kind):
    """The same table rounded to the dtype (fp16: what overflows becomes inf, an E = 255 block)."""
    delta, _ = edge_deltas()
    y = M.round_out(delta, kind)
    sent = M.round_out(np.zeros_like(delta), kind)
    for phases in ((0, 0, 0, 0), (5, 1, 3, 2)):
        _, e, _ = check(fa, torch_gpu, y, sent, kind, 0, phases, 3, "sent", "%s scale edges %s" % (kind, phases))
    assert len(set(e.tolist())) >= 6


@pytest.mark.parametrize("form", ["vector", "element"])
def test_ties_go_to_even(fa, torch_gpu, form):
    """Deltas at exactly k + 0.5 steps: a block whose maximum is 127 steps, at step 1 and at step 2^-20."""
    half = np.asarray([127.0] + [k + 0.5 for k in range(0, 15)] + [-(k + 0.5) for k in range(0, 15)] + [126.5], F32)
    delta = np.concatenate([half, np.ldexp(half, -20).astype(F32)])
    wq, we, _ = P.reply(delta, np.zeros_like(delta), "f32")
    assert list(we) == [133, 113]
    assert list(wq[1:6]) == [0, 2, 2, 4, 4] and list(wq[16:21]) == [0, -2, -2, -4, -4] and wq[31] == 126
    phases = (0, 0, 0, 0) if form == "vector" else (7, 3, 1, 2)
    check(fa, torch_gpu, delta, np.zeros_like(delta), "f32", 0, phases, 0, None, "ties, %s" % form)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["vector", "element"])
def test_non_finite_values(fa, torch_gpu, kind, form):
    """A NaN or an inf in one element makes its block E = 255, q = 0 and g' NaN throughout: in the first half of a
    block, in the second, alone in the tail's block; and an inf in the sent model that meets an inf in the new one."""
    n = 32 * 6 + 1
    y, sent = models(kind, n, 77)
    yw, sw = M.widen(y, kind).copy(), M.widen(sent, kind).copy()
    yw[3] = np.nan          # block 0, first half
    yw[32 + 20] = np.inf    # block 1, second half
    sw[64 + 9] = -np.inf    # block 2: the sent model is infinite, the delta +inf
    yw[96 + 30], sw[96 + 30] = np.inf, np.inf  # block 3: inf - inf = NaN
    yw[n - 1] = np.nan      # the tail: one element, alone in its block
    y, sent = M.round_out(yw, kind), M.round_out(sw, kind)
    wq, we, wg = P.reply(y, sent, kind)
    assert list(we[[0, 1, 2, 3, 6]]) == [255] * 5 and we[4] != 255 and we[5] != 255
    assert np.isnan(M.widen(wg, kind)[:128]).all() and np.isnan(M.widen(wg, kind)[-1]) and (wq[:128] == 0).all()
    assert np.isfinite(M.widen(wg, kind)[128:-1]).all() and wq[128:-1].any()
    phases = (0, 0, 0, 0) if form == "vector" else (9, 1, 0, 1)
    for alias in (None, "sent"):
        check(fa, torch_gpu, y, sent, kind, 0, phases, 0, alias, "%s non-finite, %s, alias %s" % (kind, form, alias))


def test_sixteen_bit_results_round_to_inf_and_land_on_subnormals(fa, torch_gpu):
    # fp16: a delta of 10000 makes the step 128; 65408 + 96 -> one step -> 65536, which rounds to inf.  A block of
    # subnormal models: the results are subnormals.
    y = np.zeros(64, F32)
    sent = np.zeros(64, F32)
    y[0], sent[0] = 5000.0, -5000.0
    y[1], sent[1] = 65504.0, 65408.0
    y[32:40] = np.arange(1, 9) * 2.0 ** -24
    sent[32:40] = np.arange(8, 0, -1) * 2.0 ** -24
    sent[41] = 2.0 ** -14
    cases = {"f16": (M.round_out(y, "f16"), M.round_out(sent, "f16"), 2.0 ** -14)}
    # bf16: u = 2^120; a delta of 255 u saturates the scale at E = 254, a step of 2 u; 252 u + 3 u -> 1.5 steps, the tie
    # goes to 2 -> 256 u = 2^128: inf
    u = 2.0 ** 120
    yb, sb = np.zeros(64, F64), np.zeros(64, F64)
    yb[0], sb[0] = 128 * u, -127 * u
    yb[1], sb[1] = 255 * u, 252 * u
    yb[32:40] = np.arange(1, 9) * 2.0 ** -133
    sb[32:40] = np.arange(8, 0, -1) * 2.0 ** -133
    sb[41] = 100 * 2.0 ** -133
    cases["bf16"] = (M.round_out(yb.astype(F32), "bf16"), M.round_out(sb.astype(F32), "bf16"), 2.0 ** -126)
    for kind, (yk, sk, tiny) in cases.items():
        assert np.array_equal(M.widen(yk, kind).astype(F64), y if kind == "f16" else yb), "the table is exact in " + kind
        wq, we, wg = P.reply(yk, sk, kind)
        w32 = M.widen(wg, kind)
        assert np.isfinite(M.widen(yk, kind)).all() and np.isfinite(M.widen(sk, kind)).all()
        assert wq[1] == (1 if kind == "f16" else 2) and np.isinf(w32[1]) and np.isfinite(w32[0])
        assert ((w32[32:40] != 0) & (np.abs(w32[32:40]) < tiny)).all()
        for phases in ((0, 0, 0, 0), (9, 1, 5, 3)):
            check(fa, torch_gpu, yk, sk, kind, 0, phases, 0, None, "%s rounding %s" % (kind, phases))


# ------------------------------------------------------------------ rule 6: the two scale modes

def scale_mode(fa, torch, y, sent, kind, idx0, e_given=None):
    """Scales only (e_given None: returns e; q and the output, handed over all the same, must stay untouched) or
    scales given (returns q, out)."""
    n, it = y.size, ITEM[kind]
    yb, sb = guarded(torch, y, (idx0 * it) % 16), guarded(torch, sent, (idx0 * it) % 16)
    qb = G.GuardedBuf(torch, n, idx0 % 16)
    ob = G.GuardedBuf(torch, n * it, (idx0 * it) % 16)
    nb = scales_touched(n, idx0)
    eb = G.GuardedBuf(torch, nb, 1) if e_given is None else guarded(torch, e_given, 1)
    before = (read(qb, U8), read(ob, U8))
    fa.mx8_encode_device(yb.ptr, sb.ptr, n, qb.ptr, eb.ptr, out=ob.ptr, dtype=fa_dt(fa, kind), idx0=idx0,
                         scales_only=e_given is None, scales_given=e_given is not None)
    torch.cuda.synchronize()
    for b in (yb, sb, qb, ob, eb):
        b.check("scale mode")
    assert np.array_equal(read(yb, U8), y.view(U8).reshape(-1)) and np.array_equal(read(sb, U8), sent.view(U8).reshape(-1))
    if e_given is None:
        assert np.array_equal(read(qb, U8), before[0]) and np.array_equal(read(ob, U8), before[1]), "scales only wrote more"
        return read(eb, U8)
    assert np.array_equal(read(eb, U8), e_given), "scales given: e is read, not written"
    return read(qb, I8), read(ob, NP_DT[kind])


@pytest.mark.parametrize("outlier", ["low", "high"])
@pytest.mark.parametrize("kind", KINDS)
def test_two_launches_share_a_block(fa, torch_gpu, kind, outlier):
    """The fused pass on [0, a) and on [a, n), a = 77 inside block 2; then on the two parts of that block scales only,
    the byte maximum, scales given.  Together: one pass over [0, n).  An outlier delta on one side of the cut makes the
    block's scale differ from the other part's own."""
    n, a = 200, 77
    y, sent = models(kind, n, 9)
    yw = M.widen(y, kind).copy()
    yw[70 if outlier == "low" else 90] += F32(0.75)
    y = M.round_out(yw, kind)
    wq, we, wg = P.reply(y, sent, kind)
    lo = encode_once(fa, torch_gpu, y[:a], sent[:a], kind, 0, (0, 0, 0, 0))
    hi = encode_once(fa, torch_gpu, y[a:], sent[a:], kind, a, vector_phases(kind, a))
    q, g = np.concatenate([lo[0], hi[0]]), np.concatenate([lo[2], hi[2]])
    e = np.concatenate([lo[1][:-1], [0], hi[1][1:]]).astype(U8)
    # the shared block: elements [64, 77) of the first launch, [77, 96) of the second
    parts = ((64, a), (a, 96))
    partial = [scale_mode(fa, torch_gpu, y[s:t], sent[s:t], kind, s) for s, t in parts]
    assert [p.size for p in partial] == [1, 1]
    assert partial[0][0] == lo[1][-1] and partial[1][0] == hi[1][0], "scales only == the fused pass's partial scale"
    E = max(partial[0][0], partial[1][0])
    assert min(partial[0][0], partial[1][0]) < E, "the outlier must change the other part's scale"
    e[2] = E
    for s, t in parts:
        q[s:t], g[s:t] = scale_mode(fa, torch_gpu, y[s:t], sent[s:t], kind, s, np.asarray([E], U8))
    assert np.array_equal(e, we), (e, we)
    assert np.array_equal(q, wq), np.flatnonzero(q != wq)[:8]
    M.assert_bits(g, wg, "two launches, %s" % kind)


def test_scale_modes_over_many_blocks(fa, torch_gpu):
    """Both modes over a whole range: scales only gives the fused pass's e, scales given under it the fused pass's q
    and g'."""
    n, idx0 = 4099, 33
    y, sent = models("f32", n, 13)
    wq, we, wg = P.reply(y, sent, "f32", idx0)
    e = scale_mode(fa, torch_gpu, y, sent, "f32", idx0)
    assert np.array_equal(e, we)
    q, g = scale_mode(fa, torch_gpu, y, sent, "f32", idx0, we)
    assert np.array_equal(q, wq)
    M.assert_bits(g, wg, "scales given")


def test_probe_and_refusals_on_the_device(fa, torch_gpu):
    t = torch_gpu.zeros(64, dtype=torch_gpu.float32, device="cuda")
    fa.mx8_encode_device(t, t, 0, t, t)  # n == 0
    with pytest.raises(fa.FaError) as ei:
        fa.mx8_encode_device(t, t.data_ptr() + 2, 4, t, t)
    assert ei.value.code == fa.ERR_ALIGN
    with fa.Aggregator(1) as agg:
        with pytest.raises(fa.FaError) as ei:
            fa.mx8_encode_device(t, t, 4, t, t, gpu=1, ctx=agg)
        assert ei.value.code == fa.ERR_ARG and "gpu" in str(ei.value)
