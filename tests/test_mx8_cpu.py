"""CPU: MX8 receipts (fa.h "MX8 receipts") -- fa_mx8_decode and fa_mx8_encode, pure host arithmetic, against
tests/mx8_ref.py bit for bit; the encoder's error bound; the n == 0 probe of fa_mx8_expand_device and its argument
errors, none of which touches a device.
"""
import numpy as np
import pytest

import mx8_ref as M

F32, F64, I8, U8, U32 = np.float32, np.float64, np.int8, np.uint8, np.uint32
MAGS = [1e-45, 1e-40, 1e-38, 1e-20, 1e-3, 1.0, 1e10, 1e30, 3e38]  # nine magnitudes, 1e-45 .. 3e38
CODES = np.arange(-128, 128).astype(I8)


def encode_cases():
    """name -> fp32 deltas: every case the encoder is checked on."""
    rng = np.random.default_rng(0x4D5838)
    cases = {}
    for mag in MAGS:
        with np.errstate(all="ignore"):
            cases["random %g" % mag] = (rng.uniform(-1, 1, 8 * 32) * mag).astype(F32)
    at = rng.uniform(-100, 100, 32).astype(F32)
    at[5] = F32(-127.0)
    cases["max at f = 127/128"] = at
    above = at.copy()
    above[5] = np.nextafter(F32(127.0), F32(np.inf))
    cases["max one ulp above"] = above
    # the same two at other exponents, the subnormal range and the top of the format included
    for sh in (-140, -126, -20, 100, 120):
        cases["max at f = 127/128, 2^%d" % sh] = np.ldexp(at, sh).astype(F32)
        cases["max one ulp above, 2^%d" % sh] = np.ldexp(above, sh).astype(F32)
    cases["ties"] = np.asarray([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, -126.5, 63.5] + [0.0] * 22, F32)
    cases["zero block"] = np.zeros(32, F32)
    cases["-0 block"] = np.full(32, -0.0, F32)
    nan = rng.uniform(-1, 1, 64).astype(F32)
    nan[7] = np.nan
    cases["one NaN"] = nan
    inf = rng.uniform(-1, 1, 64).astype(F32)
    inf[40] = -np.inf
    cases["one inf"] = inf
    cases["largest finite"] = np.asarray([np.finfo(F32).max, -np.finfo(F32).max, 1e38] + [0.0] * 29, F32)
    for n in (1, 31, 33):
        cases["n %d" % n] = rng.uniform(-3, 3, n).astype(F32)
    return cases


CASES = encode_cases()


def test_scale_bytes(fa):
    for n in (0, 1, 31, 32, 33, 64, 100003):
        assert fa.mx8_scale_bytes(n) == M.scale_bytes(n) == -(-n // 32)


def test_reference_scales_are_the_powers_of_two():
    """mx8_ref.scale against the rule: 2^(E - 133) exactly, subnormal below E = 7."""
    E = np.arange(255)
    s = M.scale(E)
    assert np.array_equal(s.astype(F64), np.ldexp(1.0, E - 133))
    assert (s[:7] < np.finfo(F32).tiny).all() and (s[7:] >= np.finfo(F32).tiny).all()
    assert np.isnan(M.scale([255])[0])


def test_decode_every_code_at_the_scale_edges(fa):
    q = np.tile(CODES, len(M.E_EDGES))
    e = np.repeat(np.asarray(M.E_EDGES, U8), 256 // 32)
    got, want = fa.mx8_decode(q, e), M.decode(q, e)
    M.assert_bits(got, want, "decode")
    # the rule itself, spelled out: exact products, but -2^128 -> -inf, and NaN at 255
    d = got.reshape(len(M.E_EDGES), 256)
    for row, E in zip(d, M.E_EDGES):
        if E == 255:
            assert np.isnan(row).all()
            continue
        exact = np.ldexp(CODES.astype(F64), E - 133)
        if E == 254:
            assert row[0] == -np.inf and exact[0] == -2.0 ** 128
            row, exact = row[1:], exact[1:]
        assert np.array_equal(row.astype(F64), exact), E


@pytest.mark.parametrize("idx0", M.IDX0S)
def test_decode_idx0_selects_the_scale(fa, idx0):
    n = 200
    rng = np.random.default_rng(idx0)
    q = rng.integers(-128, 128, n).astype(I8)
    nb = ((idx0 + n - 1) >> 5) - (idx0 >> 5) + 1
    e = rng.integers(100, 160, nb).astype(U8)
    got = fa.mx8_decode(q, e, idx0)
    M.assert_bits(got, M.decode(q, e, idx0), "idx0 %d" % idx0)
    whole_e = np.zeros(((idx0 + n - 1) >> 5) + 1, U8)
    whole_e[idx0 >> 5:] = e
    whole_q = np.zeros(idx0 + n, I8)
    whole_q[idx0:] = q
    M.assert_bits(got, M.decode(whole_q, whole_e)[idx0:], "idx0 %d against the whole bucket" % idx0)


@pytest.mark.parametrize("name", list(CASES))
def test_encode_matches_the_reference_and_its_bound(fa, name):
    delta = CASES[name]
    q, e = fa.mx8_encode(delta)
    rq, re_ = M.encode(delta)
    assert q.dtype == I8 and e.dtype == U8 and q.size == delta.size and e.size == M.scale_bytes(delta.size)
    assert np.array_equal(e, re_), (name, e, re_)
    assert np.array_equal(q, rq), (name, np.flatnonzero(q != rq)[:8])
    assert q.min(initial=0) >= -127, "the encoder never emits -128"
    # rule 4: |delta_i - d_i| <= max(m / 127, 2^-134) in every block without E = 255
    d = fa.mx8_decode(q, e)
    bound = M.error_bound(delta)
    ok = ~np.isnan(bound)
    err = np.abs(delta.astype(F64)[ok] - d.astype(F64)[ok])
    worst = np.max(err / bound[ok]) if ok.any() else 0.0
    print("%s: worst error %.4f of its bound" % (name, worst))
    assert (err <= bound[ok]).all(), (name, worst)
    assert np.isnan(d[~ok]).all() and (q[~ok] == 0).all()
    # encode . decode . encode is a fixed point
    if ok.all():
        q2, e2 = fa.mx8_encode(d)
        assert np.array_equal(e2, e) and np.array_equal(q2, q), name


def test_encode_special_blocks(fa):
    for name, E in (("zero block", 0), ("-0 block", 0)):
        q, e = fa.mx8_encode(CASES[name])
        assert (e == E).all() and (q == 0).all(), name
    q, e = fa.mx8_encode(CASES["one NaN"])
    assert list(e) == [255, M.encode(CASES["one NaN"])[1][1]] and (q[:32] == 0).all() and q[32:].any()
    q, e = fa.mx8_encode(CASES["one inf"])
    assert e[1] == 255 and e[0] != 255 and (q[32:] == 0).all()
    q, e = fa.mx8_encode(CASES["max at f = 127/128"])
    assert q[5] == -127 and e[0] == 133  # 127 = (127/128) 2^7: t = 0
    q, e = fa.mx8_encode(CASES["max one ulp above"])
    assert q[5] == 64 and e[0] == 134  # t = 1: 127.00001 / 2 rounds to 64
    q, e = fa.mx8_encode(CASES["largest finite"])
    assert e[0] == 254 and q[0] == 127 and q[1] == -127  # t would be 122: saturated at E = 254


def test_expand_probe_touches_no_device(fa):
    """n == 0 with valid arguments: FA_OK on a box without a GPU -- the feature probe."""
    for dst in (fa.F32, fa.BF16, fa.F16):
        fa.mx8_expand_device(None, None, 0, None, dst)
        fa.mx8_expand_device(None, None, 0, None, dst, ref=None, ref_dtype=fa.F32, idx0=2 ** 64 - 1)


def test_expand_argument_errors(fa):
    def refused(code, word, *a, **k):
        with pytest.raises(fa.FaError) as ei:
            fa.mx8_expand_device(*a, **k)
        assert ei.value.code == code and word in str(ei.value), (code, word, str(ei.value))

    refused(fa.ERR_ARG, "dtype", None, None, 0, None, 7)
    refused(fa.ERR_ARG, "dtype", None, None, 0, None, fa.F32, ref_dtype=-1)
    refused(fa.ERR_ARG, "bf16 slot against a f16 reference", None, None, 0, None, fa.BF16, ref_dtype=fa.F16)
    refused(fa.ERR_ARG, "f16 slot against a bf16 reference", None, None, 0, None, fa.F16, ref_dtype=fa.BF16)
    refused(fa.ERR_ARG, "2^64", None, None, 2, None, fa.F32, idx0=2 ** 64 - 1)
    refused(fa.ERR_ARG, "d_q", None, 64, 4, 256, fa.F32)
    refused(fa.ERR_ARG, "d_e", 64, None, 4, 256, fa.F32)
    refused(fa.ERR_ARG, "d_dst", 64, 64, 4, None, fa.F32)
    refused(fa.ERR_ALIGN, "slot", 64, 64, 4, 258, fa.F32)
    refused(fa.ERR_ALIGN, "slot", 64, 64, 4, 257, fa.F16)
    refused(fa.ERR_ALIGN, "reference", 64, 64, 4, 256, fa.F32, ref=1026, ref_dtype=fa.F32)
    refused(fa.ERR_ALIGN, "reference", 64, 64, 4, 256, fa.BF16, ref=1025, ref_dtype=fa.BF16)


def test_host_codec_argument_errors(fa):
    L = fa.lib()
    buf = np.zeros(64, F32)
    assert L.fa_mx8_encode(None, 4, buf.ctypes.data, buf.ctypes.data) == fa.ERR_ARG and "delta" in fa.last_error()
    assert L.fa_mx8_encode(buf.ctypes.data, 4, None, buf.ctypes.data) == fa.ERR_ARG and "q" in fa.last_error()
    assert L.fa_mx8_decode(buf.ctypes.data, None, 4, 0, buf.ctypes.data) == fa.ERR_ARG and "e" in fa.last_error()
    assert L.fa_mx8_decode(buf.ctypes.data, buf.ctypes.data, 4, 2 ** 64 - 2, buf.ctypes.data) == fa.ERR_ARG
    assert "2^64" in fa.last_error()
    assert L.fa_mx8_encode(None, 0, None, None) == fa.OK and L.fa_mx8_decode(None, None, 0, 0, None) == fa.OK
