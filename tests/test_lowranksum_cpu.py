"""CPU: the host twin of the low-rank-sum stage (fa.h "Low-rank-sum stage") against tests/lowranksum_ref.py, every bit on
lattice data; the identity with the decoder; the order of the rest chain; the probe and the refusals that need no device."""
import numpy as np
import pytest

import lowrank_ref as L
import lowranksum_ref as R

F32 = np.float32
MATS, N = L.bucket()
RANKS = [(1,), (4, 4, 4), (3, 5, 1, 64, 2)]


def receipts(ranks):
    fs = [L.lattice(MATS, N, r, 100 + 7 * c + r) for c, r in enumerate(ranks)]
    return fs, (np.arange(len(ranks)) % 8 + 1).astype(F32) / 8


@pytest.mark.parametrize("ranks", RANKS, ids=str)
@pytest.mark.parametrize("idx0,cnt", [(0, N), (MATS[3][0] + 650, 3000)])
def test_host_against_reference(fa, ranks, idx0, cnt):
    fs, w = receipts(ranks)
    R.assert_exact(fs, ranks, w, MATS, N)
    g = np.random.default_rng(1).standard_normal(N).astype(F32)
    g[MATS[1][0]:MATS[1][0] + 4] = np.array([np.nan, np.inf, -0.0, 0.0], F32)
    for ref in (None, g):
        want = R.lowrank_sum(fs, ranks, w, MATS, N, ref)[idx0:idx0 + cnt]
        got = fa.lowrank_sum_host(fs, ranks, MATS, N, w, None if ref is None else ref[idx0:idx0 + cnt], idx0, cnt)
        R.assert_bits(got, want, "ranks %s [%d, +%d) ref %s" % (ranks, idx0, cnt, ref is not None))


@pytest.mark.parametrize("r", [1, 5, 64])
def test_one_owner_of_weight_one_is_the_decoder(fa, r):
    f = L.lattice(MATS, N, r, r)
    R.assert_bits(fa.lowrank_sum_host([f], [r], MATS, N), fa.lowrank_decode(f, MATS, N, r), "D = 1, r %d" % r)


@pytest.mark.parametrize("order,want", [((0, 1, 2), 0.0), ((0, 2, 1), 1.0)])
def test_rest_chain_runs_in_client_order(fa, order, want):
    """2^24, 1, -2^24 at the first rest element: 2^24 + 1 rounds to 2^24, so the owners' order shows."""
    fs = [L.lattice(MATS, N, 1, c) for c in range(3)]
    at = L.length(MATS, N, 1) - int(L.rest_mask(MATS, N).sum())
    for c, v in zip(order, (2.0 ** 24, 1.0, -2.0 ** 24)):
        fs[c][at] = v
    a = fa.lowrank_sum_host(fs, [1, 1, 1], MATS, N)
    assert a[0] == want
    R.assert_bits(a, R.lowrank_sum(fs, [1, 1, 1], np.ones(3, F32), MATS, N), "order %s" % (order,))


@pytest.mark.parametrize("kw,code", [
    (dict(D=0), "ERR_ARG"), (dict(D=129), "ERR_ARG"), (dict(ref_dtype="BF16", out_dtype="F16"), "ERR_ARG"),
    (dict(idx0=(1 << 64) - 1, cnt=2), "ERR_ARG"), (dict(ref_dtype=7), "ERR_ARG"), (dict(cnt=8, r=0), "ERR_ARG"),
    (dict(cnt=8, r=65), "ERR_ARG"), (dict(cnt=8, out=None), "ERR_ARG"), (dict(cnt=8, f=None), "ERR_ARG"),
    (dict(cnt=8, plan=None), "ERR_ARG"), (dict(cnt=8, plan_bytes=48), "ERR_ARG"), (dict(cnt=8, f=4098), "ERR_ALIGN"),
    (dict(cnt=8, plan=4100), "ERR_ALIGN"), (dict(cnt=8, out=8194), "ERR_ALIGN"), (dict(cnt=8, ref=4098), "ERR_ALIGN"),
    (dict(cnt=8, ref=8192 + 16), "ERR_ARG")],
    ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else v)
def test_device_refusals_need_no_device(fa, kw, code):
    """Every argument is checked before any device call; cnt == 0 with valid arguments is the probe."""
    a = dict(D=2, cnt=0, idx0=0, plan=1 << 20, plan_bytes=64, f=2 << 20, r=2, ref=4096, out=8192, ref_dtype="F32", out_dtype="F32")
    fa.lowrank_sum_device(a["plan"], [a["f"]] * 2, [2, 2], 0, a["out"], plan_bytes=64, idx0=77)  # the probe
    a.update(kw)
    dt = lambda v: getattr(fa, v) if isinstance(v, str) else v
    with pytest.raises(fa.FaError) as ei:
        fa.lowrank_sum_device(a["plan"], [a["f"]] * a["D"], [a["r"]] * a["D"], a["cnt"], a["out"], dt(a["out_dtype"]), None,
                              a["ref"], dt(a["ref_dtype"]), a["idx0"], a["plan_bytes"])
    assert ei.value.code == getattr(fa, code), ei.value


def test_host_refusals_and_null_ctx(fa):
    f = L.lattice(MATS, N, 2, 0)
    for args in (([f], [65]), ([f] * 129, [2] * 129)):
        with pytest.raises((fa.FaError, ValueError)):
            fa.lowrank_sum_host(*args, MATS, N)
    with pytest.raises(fa.FaError) as ei:
        fa.lowrank_sum_host([f], [2], MATS, N, idx0=N - 1, cnt=2)
    assert ei.value.code == fa.ERR_ARG
    assert fa.LOWRANK_SUM_MAX_CLIENTS == 128
    assert fa.lib().fa_set_lowrank_sum(None, 1, None, 0, 0) == fa.ERR_ARG
    assert fa.lib().fa_submit_lowrank_sum(None, 1, 0, None, 0, 1, 1.0, 0) == fa.ERR_ARG
