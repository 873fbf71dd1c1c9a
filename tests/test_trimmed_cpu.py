"""CPU: the FA_TRIMMED reference helper (tests/trimmed_ref.py) and what libfa.so answers without a device.

The helper is checked against np.median and against hand-written columns with the expected bits written out;
the library through its constants, fa_version and the no-device probe (fa_trimmed_device with n == 0).
"""
import numpy as np
import pytest

import sort_cols as S
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


# ------------------------------------------------------------------ the structured columns (tests/sort_cols.py)

def test_the_column_families_hold_what_they_name():
    assert 16 in S.DS_EXHAUSTIVE and {2, 4, 8}.issubset(S.DS_EXHAUSTIVE)
    assert {23, 32, 47, 64}.issubset(S.DS_NETWORK) and {65, 66, 96, 127, 128}.issubset(S.DS_WIDE)
    for D in (1, 2, 5, 16):  # every pattern once
        m = S.exhaustive(D)
        assert m.shape == (D, 1 << D) and np.unique(m, axis=1).shape[1] == 1 << D
    for D in (23, 64):
        m = S.few(D)
        z = m.sum(axis=0)
        pairs = D * (D - 1) // 2
        assert m.shape[1] == 2 * (1 + D + pairs) == np.unique(m, axis=1).shape[1]
        assert [(z == v).sum() for v in (0, 1, 2, D - 2, D - 1, D)] == [1, D, pairs, pairs, D, 1]
        p = S.permutations(D, S.n_perms(D))
        assert all(sorted(p[:, r].tolist()) == list(range(D)) for r in range(p.shape[1]))
        th = S.thresholds(p)
        assert th.shape == (D, p.shape[1] * (D + 1))
        assert th.sum(axis=0).tolist() == list(range(D + 1)) * p.shape[1]
        assert np.array_equal(th[:, 5], p[:, 0] < 5)
    for D in S.DS_WIDE:  # every split of the lows between the halves, once
        m = S.wide_split(D)
        got = sorted(zip(m[:64].sum(axis=0).tolist(), m[64:].sum(axis=0).tolist()))
        assert got == [(a, b) for a in range(65) for b in range(D - 64 + 1)]
    for D in S.DS_EXHAUSTIVE + S.DS_NETWORK + S.DS_WIDE:
        m, z = S.zero_one(D)
        assert m.shape[1] % 8 == 3 and m.shape[1] < (1 << 16) + 8 and np.array_equal(z, m.sum(axis=0))
        for t in S.trims_for(D):
            assert t == T.TRIM_MEDIAN or 2 * t < D
    assert S.trims_for(128) == [0, 1, 2, 31, 62, 63, T.TRIM_MEDIAN] and S.trims_for(5) == [0, 1, 2, T.TRIM_MEDIAN]


@pytest.mark.parametrize("D", S.DS_EXHAUSTIVE + S.DS_NETWORK + S.DS_WIDE)
def test_closed_form_of_the_two_valued_columns_is_the_helper(D):
    """The closed form needs no sort; the helper sorts.  Every family, every pair, every trim (the GPU module runs
    them all on these columns)."""
    mask, z = S.zero_one(D)
    assert set(S.trims_for(D)) <= set(range((D - 1) // 2 + 1)) | {T.TRIM_MEDIAN}
    for pair in S.PAIRS01:
        xs = list(S.values(mask, pair))
        for trim in list(range((D - 1) // 2 + 1)) + [T.TRIM_MEDIAN]:
            cf = S.closed_form(D, trim, z, pair)
            assert cf.dtype == F32
            T.assert_bits(cf, T.trimmed_f32(xs, trim), "D %d %s trim %d" % (D, pair, trim))
            if pair == "nan":  # NaN exactly where a high is kept, 1.0 elsewhere
                t = T.resolve(trim, D)
                assert np.array_equal(np.isnan(cf), z < D - t) and np.all(cf[z >= D - t] == 1.0)


def test_closed_form_by_hand():
    # D = 5, trim 1: the window holds sorted positions 1..3
    z = np.arange(6)
    assert S.closed_form(5, 1, z, "01").tolist() == [1.0, 1.0, F32(2) / F32(3), F32(1) / F32(3), 0.0, 0.0]
    assert S.closed_form(5, 1, z, "pm1").tolist() == [1.0, 1.0, F32(1) / F32(3), F32(-1) / F32(3), -1.0, -1.0]
    assert np.isnan(S.closed_form(5, 1, z, "nan")).tolist() == [True, True, True, True, False, False]
    assert S.closed_form(4, 1, [2], "pm1").view(np.uint32).tolist() == [0]  # -1 + 1 = +0
    assert S.closed_form(128, T.TRIM_MEDIAN, [63, 64, 65], "01").tolist() == [1.0, 0.5, 0.0]


def test_the_structured_values_are_exact_in_16_bits():
    for D in (16, 128):
        for x in (S.perm_values(D), S.slide_columns(D)[0], S.values(S.zero_one(D)[0], "pm1")):
            assert np.array_equal(T.bf16_to_f32(T.f32_to_bf16(x.ravel())), x.ravel())
            assert np.array_equal(x.astype(np.float16).astype(F32), x)


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
