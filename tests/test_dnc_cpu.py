"""CPU: fa.dnc_select (rules 2-7 of fa.h "DnC stage") against tests/dnc_ref.py bit for bit on hand-made Gram matrices,
its argument errors, and the n == 0 probe of fa_gram_device.  No GPU."""
import numpy as np
import pytest

import dnc_ref as R

F64 = np.float64


def bits(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def gram_of(X, nan=None):
    X = np.asarray(X, F64)
    G = X @ X.T
    if nan is not None:
        G[nan, :] = G[:, nan] = np.nan
    return G


# 8 clients of 6 small-integer coordinates; clients 2 and 5 also move by one common vector
PLANTED = np.random.default_rng(0xD2C).integers(-2, 3, (8, 6)).astype(F64)
PLANTED[[2, 5]] += np.asarray([9, -9, 9, -9, 9, -9], F64)
CASES = {
    # name: (G, drop, the clients that may be deselected)
    "planted shift": (gram_of(PLANTED), 2, ([2, 5],)),
    "all equal": (gram_of(np.ones((5, 3))), 2, ([3, 4],)),  # every score +0: the highest indices go
    "nan diagonal": (gram_of(PLANTED, nan=1), 2, ([1, 2], [1, 5])),  # client 1 excluded and charged to drop
    "tie": (gram_of([[4, 0], [0, 0], [0, 0], [-4, 0], [0, 0], [0, 0]]), 1, ([3],)),  # 0 and 3 tie: the higher index goes
    "drop 0": (gram_of(PLANTED), 0, ([],)),
}


@pytest.mark.parametrize("iters", [1, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_dnc_select_is_the_reference(fa, name, iters):
    G, drop, gone = CASES[name]
    s, sel = fa.dnc_select(G, drop, iters)
    rs, rsel = R.dnc_select(G, drop, iters)
    assert np.array_equal(bits(s), bits(rs)), (name, s, rs)
    assert sel.tolist() == rsel.tolist(), (name, sel, rsel)
    assert np.flatnonzero(~sel).tolist() in gone, (name, s, sel)
    if name == "all equal":
        assert not bits(s).any(), s
    if name == "nan diagonal":
        assert s[1] == np.inf and np.isfinite(np.delete(s, 1)).all(), s
    if name == "tie":
        assert s[0] == s[3] > 0, s


@pytest.mark.parametrize("D,drop,iters,says", [(8, 4, 32, "2 drop < D"), (8, -1, 32, "0 <= drop"), (8, 2, 0, "iters = 0"),
                                               (8, 2, 1025, "iters = 1025"), (129, 2, 32, "at most 128")])
def test_dnc_select_refuses(fa, D, drop, iters, says):
    with pytest.raises(fa.FaError) as e:
        fa.dnc_select(np.eye(D), drop, iters)
    assert e.value.code == fa.ERR_ARG and says in str(e.value), str(e.value)


@pytest.mark.parametrize("D", [1, 8, 128])
def test_gram_probe_without_a_device(fa, D):
    for dt in (fa.F32, fa.BF16, fa.F16):
        g = fa.gram_device([None] * D, 0, dt)  # n == 0: FA_OK, D * D zeros, no device touched
        assert g.shape == (D, D) and not bits(g).any()
    with pytest.raises(fa.FaError) as e:
        fa.gram_device([None] * 129, 0, fa.F32)
    assert e.value.code == fa.ERR_ARG and "outside 1..128" in str(e.value)
