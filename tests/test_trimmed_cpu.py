"""CPU: the FA_TRIMMED reference helper (tests/trimmed_ref.py) and what libfa.so answers without a device.

The helper is checked against np.median and against hand-written columns with the expected bits written out;
the library through its constants, fa_version and the no-device probe (fa_trimmed_device with n == 0).
"""
import numpy as np
import pytest

import trimmed_ref as T

F32 = np.float32


def bits(*vals):
    return np.array(vals, np.uint32)


def col(*vals):
    """One element per client: D arrays of one fp32 value, given as bit patterns or floats."""
    return [np.array([v], np.uint32).view(F32) if isinstance(v, (int, np.integer)) else np.array([v], F32) for v in vals]


# ------------------------------------------------------------------ the helper

@pytest.mark.parametrize("D", [1, 3, 5, 9, 2, 4, 8])
def test_helper_is_np_median_on_finite_data(D):
    rng = np.random.default_rng(D)
    xs = [rng.uniform(-1, 1, 1001).astype(F32) for _ in range(D)]
    got = T.trimmed(xs, T.TRIM_MEDIAN)
    if D % 2:
        ref = np.median(np.stack(xs), axis=0).astype(F32)
    else:  # fl(fl(a + b) / 2) of the two middle values
        s = np.sort(np.stack(xs), axis=0)
        ref = ((s[D // 2 - 1] + s[D // 2]).astype(F32) / F32(2)).astype(F32)
        assert np.array_equal(ref.view(np.uint32), np.median(np.stack(xs), axis=0).astype(F32).view(np.uint32))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_key_transform_round_trips_and_orders():
    ordered = bits(0xFF800000, 0xFF7FFFFF, 0xBF800000, 0x80800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
                   0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000)  # -inf .. -0 +0 .. +inf
    k = T.keys(ordered.view(F32))
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(T.unkeys(k).view(np.uint32), ordered)
    nans = bits(0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)
    assert np.all(T.keys(nans.view(F32)) == 0xFFFFFFFF) and T.keys(nans.view(F32))[0] > k[-1]
    assert T.unkeys(bits(0xFFFFFFFF)).view(np.uint32)[0] == 0x7FFFFFFF


NAN, PINF, NINF, NZERO = 0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000


@pytest.mark.parametrize("column,trim,expected", [
    ((NAN, 1.0, NINF, 2.0, 3.0), 1, 0x40000000),             # NaN off the top, -inf off the bottom: (1+2+3)/3
    ((NAN, 1.0, 2.0, 3.0, 0xFFC00000), 2, 0x40400000),       # two NaNs (either sign) on top: median = 3.0
    ((NAN, 1.0, 2.0, 3.0, 4.0), 0, "nan"),                   # untrimmed NaN propagates
    ((PINF, NINF, 1.0), 0, "nan"),                           # +inf + -inf
    ((PINF, NINF, 1.0), 1, 0x3F800000),
    ((NZERO, 0.0, NZERO, 0.0), 1, 0x00000000),               # -0 < +0: kept -0, +0; +0 + -0 + +0 = +0
    ((NZERO, NZERO, NZERO), 1, 0x00000000),                  # fl(+0 + -0) = +0
    ((2.5, 2.5, 2.5, 2.5), 0, 0x40200000),                   # ties
    ((0x00000001, 0x00000003, 0x80000001), 1, 0x00000001),   # subnormals survive
    ((0x00000001, 0x00000002), 0, 0x00000002),               # fl(3 ulp / 2) ties to even: 2 ulp
    ((3e38, 3e38, -3e38, -3e38), 0, 0xFF800000),             # ascending: -3e38 + -3e38 = -inf, and it stays
    ((3e38, 3e38, -3e38, -3e38), 1, 0x00000000),             # -3e38 + 3e38 = 0
    ((0x3F800000,), T.TRIM_MEDIAN, 0x3F800000),              # D = 1: fl(fl(+0 + x) / 1)
    ((NZERO,), 0, 0x00000000),                               # D = 1, -0 -> +0
])
def test_helper_on_hand_written_columns(column, trim, expected):
    got = T.trimmed(col(*column), trim)
    if expected == "nan":
        assert np.isnan(got[0])
    else:
        assert got.view(np.uint32)[0] == expected, hex(got.view(np.uint32)[0])


def test_helper_16_bit_types():
    # fp16: subnormal inputs widen exactly; a mean beyond 65504 rounds to inf
    xs = [np.array([6e-8, 65504.0], np.float16), np.array([6e-8, 65504.0], np.float16),
          np.array([1.2e-7, 65504.0], np.float16)]
    r = T.trimmed(xs, 1, out="f16")
    assert r.view(np.uint16)[0] == np.float16(6e-8).view(np.uint16) and r[1] == np.float16(65504.0)
    big = [np.array([65504.0], F32), np.array([65536.0], F32), np.array([1e6], F32)]
    assert np.isinf(T.trimmed(big, 1, out="f16")[0])
    # bf16 bit patterns: 1.0 = 0x3F80, 3.0 = 0x4040; the mean 2.0 = 0x4000
    b = [np.array([0x3F80], np.uint16), np.array([0x4040], np.uint16)]
    assert T.trimmed(b, 0, in_bf16=True, out="bf16")[0] == 0x4000
    assert T.f32_to_bf16(np.array([1.00390625], F32))[0] == 0x3F80  # tie to even


# ------------------------------------------------------------------ the library, no device

def test_constants(fa):
    assert (fa.FEDAVG, fa.LITERAL, fa.TRIMMED) == (0, 1, 2)
    assert fa.TRIM_MEDIAN == -1


def test_abi_version_stays_7(fa):
    assert fa.lib().fa_version() == 7


def test_probe_without_a_device(fa):
    fa.trimmed_device([None] * 5, 0, fa.F32, None, fa.F32)  # n == 0: FA_OK, no device touched
    fa.trimmed_device([None] * 5, 0, fa.F32, None, fa.F32, trim=2)
    fa.trimmed_device([None], 0, fa.BF16, None, fa.BF16, trim=0)
    fa.trimmed_device([None] * fa.TRIMMED_MAX_CLIENTS, 0, fa.F16, None, fa.F32)


@pytest.mark.parametrize("D,trim,in_dt,out_dt", [
    (0, -1, "F32", "F32"),
    (129, -1, "F32", "F32"),
    (4, 2, "F32", "F32"),     # 2t >= D
    (5, 3, "F32", "F32"),
    (5, -2, "F32", "F32"),    # trim < -1
    (5, 1, "BF16", "F16"),
    (5, 1, "F16", "BF16"),
])
def test_probe_refusals(fa, D, trim, in_dt, out_dt):
    with pytest.raises(fa.FaError) as e:
        fa.trimmed_device([None] * D, 0, getattr(fa, in_dt), None, getattr(fa, out_dt), trim=trim)
    assert e.value.code == fa.ERR_ARG


def test_refusal_names_D_and_trim(fa):
    with pytest.raises(fa.FaError) as e:
        fa.trimmed_device([None] * 6, 0, fa.F32, None, fa.F32, trim=3)
    assert "6" in str(e.value) and "trim 3" in str(e.value)


def test_reduce_device_points_to_trimmed_device(fa):
    with pytest.raises(fa.FaError) as e:
        fa.reduce_device([None] * 3, [1, 1, 1], 0, fa.F32, None, fa.F32, mode=fa.TRIMMED)
    assert e.value.code == fa.ERR_ARG and "fa_trimmed_device" in str(e.value)


# ------------------------------------------------------------------ the drop-in's flags

@pytest.mark.parametrize("args,says", [
    (["--mode", "trimmed", "--trim", "2", "-d", "4"], "--trim 2"),   # 2T >= data_owners
    (["--mode", "median", "--layout", "rs"], "--layout rs"),
    (["--trim", "1"], "--mode trimmed"),                             # --trim without its mode
])
def test_aggregator_flag_refusals_exit_2(args, says):
    """Refused while the arguments are parsed: usage on stderr, exit 2, before any device or socket is opened."""
    import os
    import subprocess
    from conftest import PKG_DIR
    agg = os.path.join(PKG_DIR, "bin", "fa_aggregator")
    assert os.access(agg, os.X_OK), "build the package first"
    r = subprocess.run([agg, "-i", "-1", "-c", "1"] + args, capture_output=True, text=True, timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "usage: fa_aggregator" in r.stderr and "--mode fedavg|literal|trimmed|median" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""
