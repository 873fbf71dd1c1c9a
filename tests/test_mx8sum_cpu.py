"""CPU: the host side of the MX8-sum stage (fa.h "MX8-sum stage") against tests/mx8sum_ref.py, every bit; the order of the
chain; the refusals of fa_mx8_sum_device and of the setters that need no device."""
import numpy as np
import pytest

import mx8sum_ref as M

F32, I8, U8 = np.float32, np.int8, np.uint8
WEIGHTS = {"finite": [0.0, -0.0, -1.5, 1e-30, 2.0, 0.75], "inf": [1.0, np.inf, -2.0, 0.0, 1.0, 1.0],
           "nan": [1.0, 0.5, np.nan, 1.0, 1.0, 1.0]}


@pytest.mark.parametrize("wkind", list(WEIGHTS))
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1025])
@pytest.mark.parametrize("idx0", M.IDX0S)
def test_host_against_reference(fa, idx0, n, wkind):
    w = np.array(WEIGHTS[wkind], F32)
    q, e = M.receipts(w.size, n, idx0, 1000 * idx0 + n)
    g =np.random.default_rng(n).standard_normal(n).astype(F32)
    g[:4] = np.array([np.nan, np.inf, -0.0, 0.0], F32)[:min(4, n)]
    for ref in (None, g):
        M.assert_bits(fa.mx8_sum_host(q, e, n, w, ref, idx0), M.mx8_sum(q, e, w, idx0, ref),
                      "idx0 %d n %d %s ref %s" % (idx0, n, wkind, ref is not None))


def order_case(rev=False):
    """2^30, 1, -2^30 from three clients at element 5 (q 2^(E - 133): 64 at E = 157, 1 at E = 133): 2^30 + 1 rounds to 2^30."""
    q = [np.zeros(40, I8) for _ in range(3)]
    for c, v in enumerate((64, -64, 1) if rev else (64, 1, -64)):
        q[c][5] = v
    return q, [np.array([133 if x[5] == 1 else 157, 133], U8) for x in q], np.ones(3, F32)


@pytest.mark.parametrize("rev,want", [(False, 0.0), (True, 1.0)])
def test_order(fa, rev, want):
    q, e, w = order_case(rev)
    a = fa.mx8_sum_host(q, e, 40, w)
    assert a[5] == want and M.mx8_sum(q, e, w)[5] == want
    M.assert_bits(a, M.mx8_sum(q, e, w), "order")


@pytest.mark.parametrize("kw,code", [
    (dict(D=0), "ERR_ARG"), (dict(D=129), "ERR_ARG"), (dict(ref_dtype="BF16", out_dtype="F16"), "ERR_ARG"),
    (dict(ref_dtype="F16", out_dtype="BF16"), "ERR_ARG"), (dict(idx0=(1 << 64) - 1, n=2), "ERR_ARG"),
    (dict(ref_dtype=7), "ERR_ARG"), (dict(out_dtype=7), "ERR_ARG"), (dict(n=10, out=None), "ERR_ARG"),
    (dict(n=10, q=None), "ERR_ARG"), (dict(n=10, e=None), "ERR_ARG"), (dict(n=10, out=4096 + 66), "ERR_ALIGN"),
    (dict(n=10, ref=4096 + 2), "ERR_ALIGN"), (dict(n=10, ref=4096, out=4096 + 36), "ERR_ARG")],
    ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else v)
def test_device_refusals_need_no_device(fa, kw, code):
    """Every argument is checked before any device call, n == 0 included."""
    a = dict(D=2, n=0, idx0=0, q=1 << 20, e=2 << 20, ref=4096, out=8192, ref_dtype="F32", out_dtype="F32")
    a.update(kw)
    dt = lambda v: getattr(fa, v) if isinstance(v, str) else v
    with pytest.raises(fa.FaError) as ei:
        fa.mx8_sum_device([a["q"]] * a["D"], [a["e"]] * a["D"], a["n"], a["out"], dt(a["out_dtype"]), None, a["ref"],
                          dt(a["ref_dtype"]), a["idx0"])
    assert ei.value.code == getattr(fa, code), ei.value


def test_probe_constants_and_null_ctx(fa):
    fa.mx8_sum_device([64, 64], [64, 64], 0, 64, idx0=77)  # the probe: no device is touched
    assert (fa.MX8_SUM_MAX_CLIENTS, fa.MX8_SUM_VECTOR, fa.MX8_SUM_TILE, fa.MX8_SUM_GROUP) == (128, 1, 4096, 4)
    assert fa.mx8_sum_form(6400, [4096], 8192, fa.F32, 12288, fa.F32) == fa.MX8_SUM_VECTOR  # the rest: test_mx8sum_gpu.py
    assert fa.lib().fa_set_mx8_sum(None, 1, 1) == fa.ERR_ARG
    assert fa.lib().fa_submit_mx8_sum(None, 1, 0, None, None, 1.0, 0) == fa.ERR_ARG
