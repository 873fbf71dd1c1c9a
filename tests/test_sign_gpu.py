"""GPU: fa_sign_vote_device (fa.h "Sign-vote stage", rules 3-9) against tests/sign_ref.py, every bit (NaN as NaN), the
vote planes with their padding included.  The output lies between guard bands (tests/guarded.py) that must survive.

The cross product of the issue's axes is far too large; the covering set, stated openly:
  CLIENTS  every D of the list (the carry-save tree takes groups of 7: 6, 7, 8 and 14, 15 are its boundaries; 1, 2, 3
           partial first groups; 127, 128 the ends) at several tiles, majority with planes and mean, aligned;
  SIZES    every n of the list (word, quad of 128 and tile of 8192 edges, several tiles) at D = 8, both rules, bucket
           offset 32 * 5 (the receipts then start 4 bytes past a 16-byte boundary: a head of three words), g and the
           output at element offsets 0 and 1 (1 forces the element form);
  MARGINS  m in {1, 2, D} with and without a reference at D = 15;
  PAIRS    the six 16-bit dtype pairs and 16-bit absolute mode at D = 5 and two n, both rules;
  INPUTS   all-zero and all-one words; NaN, inf and -0 in g; receipts 8 bytes past a boundary (a range piece's phase).
"""
import numpy as np
import pytest

import guarded as G
import sign_ref as S
from test_mx8_gpu import ITEM, NP_DT, at_phase, fa_dt

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
DS = [1, 2, 3, 6, 7, 8, 14, 15, 127, 128]
NS = [1, 31, 32, 33, 127, 128, 129, 8191, 8192, 8193, 3 * 8192 + 4097]
PAIRS = [("f32", "bf16"), ("f32", "f16"), ("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32"),
         (None, "bf16"), (None, "f16")]  # (reference, output); None: absolute mode


def run_vote(fa, torch, bits, n, idx0, rule, margin, g, ref_kind, out_kind, off=0, planes=False, bphase=0, eta=0.375):
    """One call on the device against the reference; returns the form it took."""
    want, wneg, wpos = S.vote(bits, n, eta, rule, margin, None if g is None else S.widen(g, ref_kind), idx0)
    keep = [at_phase(torch, b, bphase) for b in bits]
    r_v = at_phase(torch, g, off * ITEM[ref_kind])[1] if g is not None else None
    out = G.GuardedBuf(torch, n * ITEM[out_kind], off * ITEM[out_kind])
    pl = [G.GuardedBuf(torch, S.words(n) * 4, bphase + 4 * (idx0 >> 5)) for _ in range(2)] if planes else [None, None]
    args = dict(ref=r_v, ref_dtype=fa_dt(fa, ref_kind), idx0=idx0, neg=pl[0] and pl[0].ptr, pos=pl[1] and pl[1].ptr)
    form = fa.sign_form(n, [v for _, v in keep], out.ptr, fa_dt(fa, out_kind), **args)
    fa.sign_vote_device([v for _, v in keep], n, out.ptr, fa_dt(fa, out_kind), eta, rule, margin, **args)
    torch.cuda.synchronize()
    what = "D %d n %d idx0 %d rule %d m %d %s->%s off %d form %d" % (len(bits), n, idx0, rule, margin, ref_kind, out_kind, off, form)
    S.assert_bits(out.payload().cpu().numpy().view(NP_DT[out_kind]), S.round_out(want, out_kind), what)
    out.check(what)
    for buf, plane in zip(pl, (wneg, wpos)):
        if buf is not None:
            assert np.array_equal(buf.payload().cpu().numpy().view(U32), plane), what + ": plane"
            buf.check(what)
    return form


def reference(n, kind, seed):
    return S.round_out(np.random.default_rng(seed).standard_normal(n).astype(F32), kind)


@pytest.mark.parametrize("D", DS)
def test_clients(fa, torch_gpu, D):
    n = 3 * 8192 + 4097
    bits, g = S.receipts(D, n, D), reference(n, "f32", D)
    assert run_vote(fa, torch_gpu, bits, n, 0, S.MAJORITY, 1, g, "f32", "f32", planes=True) == fa.SIGN_VECTOR
    run_vote(fa, torch_gpu, bits, n, 0, S.MEAN, 1, g, "f32", "f32")


@pytest.mark.parametrize("rule", [S.MAJORITY, S.MEAN])
@pytest.mark.parametrize("n", NS)
def test_sizes(fa, torch_gpu, n, rule):
    idx0 = 32 * 5
    bits, g = S.receipts(8, idx0 + n, n), reference(n, "f32", n)
    form = run_vote(fa, torch_gpu, bits, n, idx0, rule, 2, g, "f32", "f32", planes=rule == S.MAJORITY)
    assert form == (fa.SIGN_VECTOR if n >= 96 + 128 else fa.SIGN_ELEMENT)
    assert run_vote(fa, torch_gpu, bits, n, idx0, rule, 2, g, "f32", "f32", off=1, planes=rule == S.MAJORITY) == fa.SIGN_ELEMENT


@pytest.mark.parametrize("with_ref", [True, False])
@pytest.mark.parametrize("margin", [1, 2, 15])
def test_margins(fa, torch_gpu, margin, with_ref):
    n = 8193
    g = reference(n, "f32", margin) if with_ref else None
    run_vote(fa, torch_gpu, S.receipts(15, n, margin), n, 0, S.MAJORITY, margin, g, "f32", "f32", planes=True)
    run_vote(fa, torch_gpu, S.receipts(15, n, margin), n, 0, S.MEAN, margin, g, "f32", "f32")


@pytest.mark.parametrize("rule", [S.MAJORITY, S.MEAN])
@pytest.mark.parametrize("pair", PAIRS, ids=["%s->%s" % (r or "abs", o) for r, o in PAIRS])
def test_dtype_pairs(fa, torch_gpu, pair, rule):
    ref_kind, out_kind = pair
    for n in (129, 8192 + 257):
        g = reference(n, ref_kind, n) if ref_kind else None
        if g is not None and ref_kind != "bf16":
            g[:3] = [6e-8, 65504.0, -6e-5]  # an fp16 subnormal, the largest fp16, a value whose sum is subnormal
        for off in (0, 1):
            run_vote(fa, torch_gpu, S.receipts(5, n, n + off), n, 0, rule, 1, g, ref_kind or out_kind, out_kind, off=off,
                     eta=6e-5)


@pytest.mark.parametrize("rule", [S.MAJORITY, S.MEAN])
def test_inputs(fa, torch_gpu, rule):
    n, D = 8192 + 300, 4
    planes = rule == S.MAJORITY
    g = reference(n, "f32", 1)
    g[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], F32), g[::7].size)
    for fill in (False, True):  # every count 0, every count D
        run_vote(fa, torch_gpu, [S.to_plane(np.full(n, fill))] * D, n, 0, rule, 2, g, "f32", "f32", planes=planes)
    run_vote(fa, torch_gpu, S.receipts(D, n, 3), n, 0, rule, 1, g, "f32", "f32", planes=planes)
    # a range piece's phase: receipts and planes 8 bytes past a 16-byte boundary (a head of two words)
    assert run_vote(fa, torch_gpu, S.receipts(D, n, 4), n, 0, rule, 1, g, "f32", "f32", planes=planes, bphase=8) == fa.SIGN_VECTOR
