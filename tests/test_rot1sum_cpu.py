"""CPU: the host side of the rot1-sum stage (fa.h "Rot1-sum stage") against tests/rot1sum_ref.py, every bit; the derived
bound against fp64; the exact identities; the order of groups and owners; the refusals that need no device."""
import numpy as np
import pytest

import rot1sum_ref as R

F32, U32 = np.float32, np.uint32
SEEDS = {"one seed": [7] * 6, "all distinct": [11, 12, 13, 14, 15, 16], "A B A": [7, 9, 7, 9, 7, 7]}
W = np.array([1.0, -0.5, 0.25, 1.5, -2.0, 0.75], F32)


@pytest.mark.parametrize("pattern", list(SEEDS))
@pytest.mark.parametrize("cnt", [1, 4097, 2 * 4096 + 2049])
@pytest.mark.parametrize("idx0", [0, 64, 205, 4096 + 192])
def test_host_against_restatement_and_bound(fa, idx0, cnt, pattern):
    bits, scale, _ = R.receipts(fa, 6, cnt, idx0, idx0 + cnt)
    seed = SEEDS[pattern]
    g = np.random.default_rng(cnt).standard_normal(cnt).astype(F32)
    g[:4] = np.array([np.nan, np.inf, -0.0, 0.0], F32)[:min(4, cnt)]
    for ref in (None, g):
        parts = []
        want = R.rot1_sum(fa, bits, scale, seed, W, cnt, idx0, ref, parts)
        R.assert_bits(fa.rot1_sum_host(bits, scale, seed, cnt, W, ref, idx0), want, "%s idx0 %d cnt %d" % (pattern, idx0, cnt))
        ok = np.isfinite(want)  # NaN blocks and inf references have no bound
        with np.errstate(all="ignore"):
            err = np.abs(want.astype(np.float64) - R.exact(fa, bits, scale, seed, W, cnt, idx0, ref))
        assert (ok.any() or cnt == 1) and np.all(err[ok] <= R.bound(parts, cnt, idx0, ref)[ok])  # cnt 1: a NaN block


def test_one_owner_is_the_decoder(fa):
    """Rule 8: w = 1 and scales of 12 significant bits: the decoder's values, every partial sum exact; rule 5 starts from
    +0, so the decoder's -0 comes out +0."""
    n = 4096 + 300
    bits, scale, _ = R.receipts(fa, 1, n, 0, 3, edges=False)
    scale = [(np.array([0x801, 0xfff], F32) * F32(2.0 ** -20))]
    R.assert_bits(fa.rot1_sum_host(bits, scale, 7, n), fa.rot1_decode(bits[0], scale[0], 7, n) + F32(0.0), "one owner")


def test_small_integers_are_exact(fa):
    n, D = 4096 + 300, 8
    bits, scale, _ = R.receipts(fa, D, n, 0, 4, edges=False)
    rng = np.random.default_rng(1)
    scale = [(rng.integers(1, 17, 2) * 2.0 ** -9).astype(F32) for _ in range(D)]
    w = np.array([1, 2, 0.5, -1, -2, 1, 0.5, 2], F32)
    assert np.array_equal(fa.rot1_sum_host(bits, scale, 7, n, w).astype(np.float64), R.exact(fa, bits, scale, 7, w, n))


@pytest.mark.parametrize("seed", [[7, 7, 7], [1, 2, 3]], ids=["within a group", "groups"])
def test_order(fa, seed):
    """t = 2^30, 1, -2^30: where the large terms cancel, the small one survives only if it is added last."""
    bits, _, _ = R.receipts(fa, 3, 4096, 0, 5, edges=False)
    bits = [bits[0], bits[1], bits[0]] if seed[0] == seed[2] else bits
    scale, w = [np.array([s], F32) for s in (2.0 ** 30, 1.0, 2.0 ** 30)], np.array([1, 1, -1], F32)
    swap = [0, 2, 1]
    a = fa.rot1_sum_host(bits, scale, seed, 4096, w)
    b = fa.rot1_sum_host([bits[i] for i in swap], [scale[i] for i in swap], [seed[i] for i in swap], 4096, w[swap])
    assert not np.array_equal(a, b)
    R.assert_bits(a, R.rot1_sum(fa, bits, scale, seed, w, 4096), "order")
    R.assert_bits(b, R.rot1_sum(fa, [bits[i] for i in swap], [scale[i] for i in swap], [seed[i] for i in swap], w[swap], 4096),
                  "swapped")


@pytest.mark.parametrize("kw,code", [
    (dict(D=0), "ERR_ARG"), (dict(D=129), "ERR_ARG"), (dict(ref_dtype="BF16", out_dtype="F16"), "ERR_ARG"),
    (dict(idx0=(1 << 64) - 1, n=2), "ERR_ARG"), (dict(ref_dtype=7), "ERR_ARG"), (dict(n=10, out=None), "ERR_ARG"),
    (dict(n=10, bits=None), "ERR_ARG"), (dict(n=10, scale=None), "ERR_ARG"), (dict(n=10, bits=4098), "ERR_ALIGN"),
    (dict(n=10, out=4096 + 66), "ERR_ALIGN"), (dict(n=10, ref=4096 + 2), "ERR_ALIGN"), (dict(n=10, ref=4096, out=4096 + 36), "ERR_ARG")],
    ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else v)
def test_device_refusals_need_no_device(fa, kw, code):
    """Every argument is checked before any device call, cnt == 0 included."""
    a = dict(D=2, n=0, idx0=0, bits=1 << 20, scale=2 << 20, ref=4096, out=8192, ref_dtype="F32", out_dtype="F32")
    a.update(kw)
    dt = lambda v: getattr(fa, v) if isinstance(v, str) else v
    with pytest.raises(fa.FaError) as ei:
        fa.rot1_sum_device([a["bits"]] * a["D"], [a["scale"]] * a["D"], 7, a["n"], a["out"], dt(a["out_dtype"]), None, a["ref"],
                           dt(a["ref_dtype"]), a["idx0"])
    assert ei.value.code == getattr(fa, code), ei.value


def test_probe_constants_and_null_ctx(fa):
    fa.rot1_sum_device([64, 64], [64, 64], [1, 2], 0, 64, idx0=77)  # the probe: no device is touched
    assert (fa.ROT1_SUM_MAX_CLIENTS, fa.ROT1_SUM_DEPTH) == (128, 8)
    assert fa.lib().fa_set_rot1_sum(None, 1, 1) == fa.ERR_ARG
    assert fa.lib().fa_submit_rot1_sum(None, 1, 0, None, None, 7, 1.0, 0) == fa.ERR_ARG
