"""CPU: the host side of the sign-vote stage (fa.h "Sign-vote stage") against tests/sign_ref.py, every bit, and the
refusals of fa_sign_vote_device that need no device."""
import numpy as np
import pytest

import sign_ref as S

F32, U32 = np.float32, np.uint32


def test_pack_rule(fa):
    d = np.array([-1.0, 1.0, -0.0, 0.0, np.nan, -np.inf, np.inf, -1e-45] * 5, F32)
    got = fa.sign_pack(d)
    assert np.array_equal(got, S.pack(d)) and got.size == fa.sign_words(d.size) == 2
    assert S.unpack(got, 0, 8).tolist() == [1, 0, 0, 0, 0, 1, 0, 1] and got[1] >> 8 == 0  # -0 and NaN clear, padding 0


@pytest.mark.parametrize("rule", [S.MAJORITY, S.MEAN])
@pytest.mark.parametrize("D", [1, 4, 7, 128])
def test_vote_host(fa, D, rule):
    n, idx0 = 1000 + D, 64
    bits = S.receipts(D, idx0 + n, D * 7 + rule)
    g = np.random.default_rng(D).standard_normal(n).astype(F32)
    g[:4] = [np.nan, np.inf, -0.0, 0.0]
    for margin in sorted({1, min(2, D), D}):
        for ref in (None, g):
            want, wneg, wpos = S.vote(bits, n, 0.125, rule, margin, ref, idx0)
            what = "D %d rule %d m %d ref %s" % (D, rule, margin, ref is not None)
            if rule == S.MAJORITY:
                got, neg, pos = fa.sign_vote_host(bits, n, 0.125, rule, margin, ref, idx0, planes=True)
                assert np.array_equal(neg, wneg) and np.array_equal(pos, wpos), what
            else:
                got = fa.sign_vote_host(bits, n, 0.125, rule, margin, ref, idx0)
            S.assert_bits(got, want, what)


def test_tie_and_padding(fa):
    """A tie on even D gives +0 (also against g = -0) and clears both plane bits; padding bits set to 1 change nothing."""
    n = 40
    bits = [S.to_plane(np.ones(n, bool)), S.to_plane(np.zeros(n, bool))]
    a, neg, pos = fa.sign_vote_host(bits, n, 1.0, S.MAJORITY, 1, np.full(n, -0.0, F32), planes=True)
    assert not a.view(U32).any() and not neg.any() and not pos.any()
    dirty = [b.copy() for b in S.receipts(3, n, 1)]
    clean = fa.sign_vote_host(dirty, n, 1.0, S.MAJORITY, 1, None, planes=True)
    for b in dirty:
        b[1] |= U32(0xFFFFFF00)
    for x, y in zip(fa.sign_vote_host(dirty, n, 1.0, S.MAJORITY, 1, None, planes=True), clean):
        assert np.array_equal(x.view(U32), y.view(U32))


@pytest.mark.parametrize("kw", [dict(idx0=33), dict(margin=0), dict(margin=3), dict(D=0), dict(D=129), dict(eta=np.nan),
                                dict(eta=np.inf), dict(eta=0.0), dict(eta=-1.0), dict(neg=64), dict(pos=64), dict(rule=2),
                                dict(neg=64, pos=64, rule=S.MEAN), dict(ref_dtype="BF16", out_dtype="F16"),
                                dict(ref_dtype="F16", out_dtype="BF16")],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_device_refusals_need_no_device(fa, kw):
    """Every argument is checked before any device call, n == 0 included: FA_ERR_ARG."""
    a = dict(D=2, n=0, eta=1.0, rule=S.MAJORITY, margin=1, idx0=0, neg=None, pos=None, ref_dtype="F32", out_dtype="F32")
    a.update(kw)
    with pytest.raises(fa.FaError) as e:
        fa.sign_vote_device([64] * a["D"], a["n"], 64, getattr(fa, a["out_dtype"]), a["eta"], a["rule"], a["margin"], None,
                            getattr(fa, a["ref_dtype"]), a["idx0"], a["neg"], a["pos"])
    assert e.value.code == fa.ERR_ARG, e.value


def test_probe(fa):
    fa.sign_vote_device([64, 64], 0, 64, fa.F32, 1.0, fa.SIGN_MAJORITY, 2, None, fa.F32, 32 * 5)
    assert (fa.SIGN_MAJORITY, fa.SIGN_MEAN, fa.SIGN_MAX_CLIENTS) == (0, 1, 128)
