"""CPU: the host side of the sparse-sum stage (fa.h "Sparse-sum stage") against tests/sparse_ref.py, every bit; the
reference's fmaf against the oracle's chain; the refusals of fa_sparse_sum_device that need no device."""
import numpy as np
import pytest

import sparse_ref as S

F32, U32 = np.float32, np.uint32
E_SMALL, E_BIG = 2048, 8192
NS = sorted({1, 15, 16, 17} | {e + d for e in (E_SMALL, E_BIG) for d in (-1, 0, 1)} | {3 * E_SMALL + E_SMALL // 2 + 1})


def dense(D, n, seed):
    """D dense updates whose chain is order-sensitive, with the IEEE edges in front, and mixed-sign weights."""
    rng = np.random.default_rng(seed)
    xs = [(rng.standard_normal(n) * 2.0 ** (8 * c % 40)).astype(F32) for c in range(D)]
    for c, x in enumerate(xs):
        x[:6] = np.roll(np.array([np.nan, np.inf, -0.0, 0.0, 1e-45, -1e-45], F32), c)[:min(6, n)]
    w = (rng.standard_normal(D) * np.where(np.arange(D) % 3, 1.0, -1.0)).astype(F32)
    return xs, w


@pytest.mark.parametrize("D", [1, 3, 16])
def test_reference_fmaf_is_the_oracles(O, D):
    n = 5000
    xs, w = dense(D, n, D)
    acc = np.zeros(n, F32)
    for x, wk in zip(xs, w):
        acc = S.fmaf(wk, x, acc)
    S.assert_bits(acc, O.fedavg(xs, w), "D %d" % D)


@pytest.mark.parametrize("D", [1, 5, 128])
@pytest.mark.parametrize("n", NS)
def test_host_against_reference(fa, n, D):
    idx0 = 77
    idx, val = S.receipts(D, idx0 + n + 99, max(1, n // 8), n + D, empty={1})
    w = np.random.default_rng(D).standard_normal(D).astype(F32)
    g = np.random.default_rng(n).standard_normal(n).astype(F32)
    g[:4] = np.array([np.nan, np.inf, -0.0, 0.0], F32)[:min(4, n)]
    for ref in (None, g):
        S.assert_bits(fa.sparse_sum_host(idx, val, n, w, ref, idx0), S.sparse_sum(idx, val, w, n, idx0, ref),
                      "D %d n %d ref %s" % (D, n, ref is not None))


@pytest.mark.parametrize("D", [2, 7, 16])
def test_full_receipts_are_the_fedavg_chain(fa, O, D):
    """k_c = n for every client, absolute mode: the oracle's FA_FEDAVG chain on the dense deltas, bit for bit."""
    n = 3001
    xs, w = dense(D, n, 100 + D)
    got = fa.sparse_sum_host([np.arange(n, dtype=U32)] * D, xs, n, w)
    S.assert_bits(got, O.fedavg(xs, w), "D %d" % D)


def test_minus_zero_and_unnamed_elements(fa):
    """A partial sum of -0 (an underflowing product) stays -0 across a client that skips the element; the add of rule 2
    is done where nobody named the element: -0 + +0 = +0."""
    idx, val = [np.array([0, 1], U32), np.array([2], U32)], [np.array([-1e-30, 0.0], F32), np.array([1.0], F32)]
    w = np.array([1e-30, -1.0], F32)
    a = fa.sparse_sum_host(idx, val, 4, w)
    assert a.view(U32).tolist() == [0x80000000, 0, 0xBF800000, 0]
    S.assert_bits(a, S.sparse_sum(idx, val, w, 4), "absolute")
    g = np.full(4, -0.0, F32)
    assert fa.sparse_sum_host(idx, val, 4, w, g).view(U32).tolist() == [0x80000000, 0, 0xBF800000, 0]


@pytest.mark.parametrize("kw", [dict(D=0), dict(D=129), dict(ref_dtype="BF16", out_dtype="F16"), dict(k=1 << 32),
                                dict(ref_dtype="F16", out_dtype="BF16"), dict(idx0=(1 << 64) - 1, n=2),
                                dict(idx0=1 << 32, n=1, k=1), dict(ref_dtype=7), dict(out_dtype=7)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_device_refusals_need_no_device(fa, kw):
    """Every argument is checked before any device call, n == 0 included: FA_ERR_ARG."""
    a = dict(D=2, n=0, idx0=0, k=0, ref_dtype="F32", out_dtype="F32")
    a.update(kw)
    dt = lambda v: getattr(fa, v) if isinstance(v, str) else v
    with pytest.raises(fa.FaError) as e:
        fa.sparse_sum_device([64] * a["D"], [64] * a["D"], [a["k"]] * a["D"], a["n"], 64, 64, dt(a["out_dtype"]), None, 64,
                             dt(a["ref_dtype"]), a["idx0"])
    assert e.value.code == fa.ERR_ARG, e.value


@pytest.mark.parametrize("kw,code", [(dict(out=None), "ERR_ARG"), (dict(work=None), "ERR_ARG"), (dict(idx=None), "ERR_ARG"),
                                     (dict(out=66), "ERR_ALIGN"), (dict(ref=66), "ERR_ALIGN"), (dict(idx=66), "ERR_ALIGN"),
                                     (dict(val=66), "ERR_ALIGN"), (dict(work=72), "ERR_ALIGN"),
                                     (dict(ref=4096, out=4096 + 36), "ERR_ARG")],
                         ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else v)
def test_pointer_refusals_need_no_device(fa, kw, code):
    """Null pointers, alignment and the overlap of d_out with d_ref are refused before any device call (n > 0)."""
    a = dict(idx=1 << 20, val=2 << 20, out=4096 + 64, ref=4096, work=3 << 20)
    a.update(kw)
    with pytest.raises(fa.FaError) as e:
        fa.sparse_sum_device([a["idx"]], [a["val"]], [3], 10, a["out"], a["work"], fa.F32, None, a["ref"], fa.F32)
    assert e.value.code == getattr(fa, code), e.value


def test_probe_and_forms(fa):
    fa.sparse_sum_device([64, 64], [64, 64], [0, 5], 0, 64, 64, fa.F32, None, None, fa.F32, 77)
    assert fa.SPARSE_MAX_CLIENTS == 128 and fa.SPARSE_TILES == (E_SMALL, E_BIG)
    assert fa.sparse_sum_workspace(1, 1) >= 8 and fa.sparse_sum_workspace(E_SMALL + 1, 128) >= 128 * 3 * 4
    # the tile by density (below 1 / 2048: the big one), the vector bit by the common head of g and the output
    assert fa.sparse_sum_form(6400, [3, 3], 4096, fa.F32, 8192, fa.F32) == fa.SPARSE_VECTOR | fa.SPARSE_BIG_TILE
    assert fa.sparse_sum_form(6400, [100, 100], 4096 + 4, fa.F32, 8192 + 4, fa.F32) == fa.SPARSE_VECTOR
    assert fa.sparse_sum_form(6400, [100, 100], 4096, fa.F32, 8192 + 4, fa.F32) == 0
    assert fa.sparse_sum_form(6400, [0], 4096 + 2, fa.BF16) == fa.SPARSE_VECTOR | fa.SPARSE_BIG_TILE
