"""CPU: the Bulyan stage's numpy helper (tests/bulyan_ref.py) against a brute force and on hand-written columns,
fa_bulyan_select against it, the no-device probes and refusals of the library, and the drop-in's --mode bulyan
flags."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import bulyan_ref as B
import sort_cols as S
import trimmed_ref as T

F32, F64 = np.float32, np.float64
INF, NAN = math.inf, math.nan


def bits32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32).tolist()


def bits64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64).tolist()


def one(vals, keep):
    """Rule 4 on one column: (the result, the window start j)."""
    r, j = B.centered_f32([np.asarray([v], F32) for v in vals], keep)
    return r[0], int(j[0])


# ------------------------------------------------------------------ rule 4: the helper

def test_helper_is_the_nearest_to_the_median_on_finite_tie_free_columns():
    """Brute force: the `keep` sorted values with the smallest distance to the median (below it: to the lower
    median, above it: to the upper one), the lower position first where both medians tie at 0.  Distinct integers
    below 2^17 whose non-zero distances are distinct too: no rounding and no other tie is involved."""
    rng = np.random.default_rng(0xB017)
    cols = mism = 0
    for theta in range(1, 40):
        for keep in range(1, theta + 1):
            for _ in range(5):
                while True:
                    s = np.sort(rng.choice(100_000, theta, replace=False)).astype(np.int64)
                    c_lo, c_hi = s[(theta - 1) // 2], s[theta // 2]
                    dist = np.where(np.arange(theta) <= (theta - 1) // 2, c_lo - s, s - c_hi)
                    nz = dist[dist > 0]
                    if len(set(nz.tolist())) == nz.size:
                        break
                picked = np.sort(np.argsort(dist, kind="stable")[:keep])
                expect = F32(0.0)
                for u in picked:
                    expect = F32(expect + F32(s[u]))
                expect = F32(expect / F32(keep))
                got, j = one(rng.permutation(s).astype(F32), keep)
                cols += 1
                if not (picked.tolist() == list(range(j, j + keep)) and bits32(got) == bits32(expect)):
                    mism += 1
    assert cols == 3900 and mism == 0, (cols, mism)


def test_keep_theta_is_the_trimmed_mean_with_trim_0():
    rng = np.random.default_rng(3)
    for theta in (1, 2, 5, 8, 33):
        xs = [rng.normal(size=67).astype(F32) for _ in range(theta)]
        r, j = B.centered_f32(xs, theta)
        assert not j.any() and bits32(r) == bits32(T.trimmed_f32(xs, 0))


def test_hand_written_columns():
    tiny = float(F32(2.0 ** -149))
    # duplicates and ties keep the lower window
    assert one([1, 1, 2, 2, 3], 3) == (F32(F32(1 + 2 + 2) / F32(3)), 1)  # then 3 - 2 < 2 - 1 is false: a tie
    assert one([1, 1, 1, 1, 1], 2) == (F32(1.0), 0)
    assert one([0, 1, 2, 3, 4], 3) == (F32(2.0), 1) and one([0, 1, 2, 3, 4], 1) == (F32(2.0), 2)
    assert one([0, 1, 2, 3], 2) == (F32(1.5), 1)   # even theta: both medians
    assert one([0, 1, 2, 3], 1) == (F32(1.0), 1)   # the tie between the two medians: the lower one
    assert one([0, 1, 2, 3], 3) == (F32(1.0), 0)   # d_hi = 3 - 2, d_lo = 1 - 0: a tie, the lower window
    # signed zeros: -0 sorts below +0, every difference is +0, nothing slides; +0 + -0 = +0
    r, j = one([0.0, -0.0, 0.0, -0.0], 2)
    assert bits32(r) == [0] and j == 0
    # subnormal differences are kept: 3 tiny - 2 tiny < 2 tiny - (-tiny)
    r, j = one([-tiny, 0.0, 2 * tiny, 3 * tiny, 9 * tiny], 3)
    assert j == 1 and r == F32(F32(5 * tiny) / F32(3))
    # +inf at the top is never slid into; -inf at the bottom is slid away when the centre is finite
    assert one([INF, 1, 2, 3, -1], 3) == (F32(2.0), 1)
    assert one([-INF, 1, 2, 3, 5], 3) == (F32(2.0), 1)
    assert one([-INF, 1, 2, 3, 5], 4) == (F32(F32(1 + 2 + 3 + 5) / F32(4)), 1)
    r, j = one([-INF, -INF, -INF, 1, 2], 3)  # the centre is -inf: d_lo = -inf - -inf = NaN, no slide
    assert j == 0 and r == -INF
    # one NaN sorts above +inf and stays out while keep < theta; with keep == theta it is in the sum
    assert one([NAN, 0, 1, 2, 3], 3) == (F32(2.0), 1)
    assert math.isnan(one([NAN, 0, 1, 2, 3], 5)[0])
    # more NaNs than half: the centre is NaN, every comparison is false, the window stays at the bottom
    r, j = one([NAN, NAN, NAN, 1, 2], 2)
    assert j == 0 and r == F32(1.5)
    r, j = one([NAN, NAN, NAN, 1, 2], 3)
    assert j == 0 and math.isnan(r)
    # 3e38 - (-3e38) overflows to +inf (only d_lo can: c_lo <= c_hi): the low value is slid away like a -inf
    assert one([-3e38, 1, 2, 3, 3e38], 3) == (F32(2.0), 1)
    assert one([-3e38, 3e38, 3e38], 1) == (F32(3e38), 1)
    r, j = one([-3e38, -3e38, 3e38, 3e38], 2)  # both differences are 0: no slide; the sum overflows
    assert j == 0 and r == -INF
    # theta = 1 and 2
    assert one([7], 1) == (F32(7.0), 0) and one([1, 4], 1) == (F32(1.0), 0) and one([1, 4], 2) == (F32(2.5), 0)


def test_special_columns_cover_every_class():
    for theta in (1, 2, 3, 9, 128):
        cols = B.special_columns(theta)
        assert all(c.shape == (theta,) and c.dtype == F32 for c in cols)
        flat = np.concatenate(cols)
        assert np.isnan(flat).any() and np.isinf(flat).any()
        if theta >= 2:
            assert (flat.view(np.uint32) == 0x80000000).any()
            assert ((np.abs(flat) > 0) & (np.abs(flat) < 2.0 ** -126)).any()


def test_a_16_bit_output_is_rounded_once():
    xs = [np.asarray([1.0], F32), np.asarray([1.0 + 2.0 ** -8], F32), np.asarray([1.0 + 2.0 ** -7], F32)]
    assert B.centered(xs, 3, "f32", "bf16").tolist() == T.f32_to_bf16(B.centered_f32(xs, 3)[0]).tolist()
    assert B.centered(xs, 3, "f32", "f16").dtype == np.float16


# ------------------------------------------------------------------ rule 4 on the structured columns (sort_cols.py)

@pytest.mark.parametrize("theta", S.SLIDE_THETAS)
def test_slide_columns_reach_every_window_start_and_no_other(theta):
    """Through the j the helper returns: at every keep the GPU module runs (all of 1..theta), column `target`
    starts at min(target, theta - keep), so the starts are exactly 0..min(theta - keep, (theta - 1) // 2)."""
    x, target = S.slide_columns(theta)
    assert sorted(set(target.tolist())) == list(range((theta - 1) // 2 + 1))
    for kind in ("bf16", "f16"):  # the 16-bit runs see the same values
        assert bits32(B.widen(B.round_out(x.ravel(), kind), kind)) == bits32(x.ravel())
    for keep in range(1, theta + 1):
        _, j = B.centered_f32(list(x), keep)
        assert np.array_equal(j, np.minimum(target, theta - keep)), (theta, keep)
        assert sorted(set(j.tolist())) == S.slide_targets(theta, keep), (theta, keep)


def test_slide_targets_by_hand():
    assert S.slide_targets(7, 7) == [0] and S.slide_targets(7, 5) == [0, 1, 2] and S.slide_targets(7, 1) == [0, 1, 2, 3]
    assert S.slide_targets(64, 1) == list(range(32)) and S.slide_targets(64, 40) == list(range(25))
    assert one([-1024, 1, -1032, 1, 1, 1, 1], 3) == (F32(1.0), 2)


@pytest.mark.parametrize("D", [5, 16, 23, 64, 65, 128])
def test_two_valued_columns_with_keep_theta_have_the_trim_0_closed_form(D):
    mask, z = S.zero_one(D)
    for pair in S.PAIRS01:
        r, j = B.centered_f32(list(S.values(mask, pair)), D)
        assert not j.any()
        T.assert_bits(r, S.closed_form(D, 0, z, pair), "D %d %s" % (D, pair))


# ------------------------------------------------------------------ rule 2: the helper and fa_bulyan_select

def sym(rows):
    Q = np.asarray(rows, F64)
    assert Q.shape[0] == Q.shape[1] and bits64(Q) == bits64(Q.T)
    return Q


def check_against_helper(fa, Q, f):
    order, ps, sel = fa.bulyan_select(Q, f)
    rorder, rps, rsel = B.select(Q, f)
    assert order.tolist() == rorder.tolist(), (Q.shape, f, order, rorder)
    assert bits64(ps) == bits64(rps), (Q.shape, f, ps, rps)
    assert sel.tolist() == rsel.tolist()
    return order, ps, sel


def test_helper_selection_by_hand():
    # D = 3, f = 0: c = 1, 1, then a lone client that scores +0
    Q = sym([[0, 1, 9], [1, 0, 4], [9, 4, 0]])
    order, ps, sel = B.select(Q, 0)
    assert order.tolist() == [0, 1, 2] and ps.tolist() == [1.0, 4.0, 0.0] and sel.all()
    # a far owner is picked last or not at all: D = 7, f = 1 picks 5, never owner 6
    Q = np.ones((7, 7))
    Q[6, :] = Q[:, 6] = 100.0
    np.fill_diagonal(Q, 0.0)
    order, ps, sel = B.select(sym(Q), 1)
    assert order.tolist() == [0, 1, 2, 3, 4] and not sel[6] and not sel[5]
    assert ps.tolist() == [4.0, 3.0, 2.0, 1.0, 1.0]  # c = 4, 3, 2, 1, max(1, 0)


def test_abi_version_stays_7(fa):
    assert fa.lib().fa_version() == 7


@pytest.mark.parametrize("D", [3, 4, 7, 8, 11, 33, 67, 128])
def test_fa_bulyan_select_is_the_helper_on_random_matrices(fa, D):
    rng = np.random.default_rng(0xB1A + D)
    fmax = (D - 3) // 4
    for case in range(24 if D <= 33 else 6):
        A = 10.0 ** rng.uniform(-6, 6, (D, D))
        if case % 3 == 1:  # few distinct values: many ties
            A = rng.integers(0, 4, (D, D)).astype(F64)
        Q = np.triu(A, 1)
        Q = Q + Q.T
        if case % 4 == 2:  # NaN / inf rows
            for k in rng.choice(D, max(1, D // 4), replace=False):
                Q[k, :] = Q[:, k] = rng.choice([NAN, INF])
            np.fill_diagonal(Q, 0.0)
        if case % 4 == 3:  # single NaN / inf entries
            for _ in range(D):
                a, b = rng.choice(D, 2, replace=False)
                Q[a, b] = Q[b, a] = rng.choice([NAN, INF])
        Q = sym(Q)
        for f in sorted({0, fmax, int(rng.integers(0, fmax + 1))}):
            check_against_helper(fa, Q, f)


def test_fa_bulyan_select_nan_rows_all_inf_and_the_empty_last_row(fa):
    Q = sym([[0, 1, 9], [1, 0, 4], [9, 4, 0]])
    order, ps, sel = check_against_helper(fa, Q, 0)  # D = 3, f = 0: the last pick has an empty row
    assert order.tolist() == [0, 1, 2] and bits64(ps) == bits64([1.0, 4.0, 0.0])
    for D, f in ((3, 0), (7, 1), (11, 2)):
        Q = np.full((D, D), INF)
        np.fill_diagonal(Q, 0.0)
        order, ps, sel = check_against_helper(fa, sym(Q), f)  # every row +inf: nothing is picked
        assert order.size == 0 and ps.size == 0 and not sel.any()
        Q = np.full((D, D), NAN)
        np.fill_diagonal(Q, 0.0)
        order, ps, sel = check_against_helper(fa, sym(Q), f)
        assert order.size == 0 and not sel.any()
    # one NaN row among seven, f = 1: theta = 5 of the six others are picked, the NaN owner never
    Q = np.abs(np.subtract.outer(np.arange(7.0), np.arange(7.0)))
    Q[2, :] = Q[:, 2] = NAN
    np.fill_diagonal(Q, 0.0)
    order, ps, sel = check_against_helper(fa, sym(Q), 1)
    assert len(order) == 5 and 2 not in order.tolist()
    # two NaN rows, more than f: the last honest owner left has only NaN neighbours, scores +inf and ends the
    # selection one short of theta
    Q[5, :] = Q[:, 5] = NAN
    np.fill_diagonal(Q, 0.0)
    order, ps, sel = check_against_helper(fa, sym(Q), 1)
    assert len(order) == 4 and not sel[2] and not sel[5]
    # the unused entries of the C arrays: -1 and +inf
    D = 7
    o, s, fl = np.zeros(D, np.intc), np.zeros(D, F64), np.zeros(D, np.intc)
    ns = ctypes.c_int(-1)
    Q = sym(Q)
    assert fa.lib().fa_bulyan_select(Q.ctypes.data, D, 1, o.ctypes.data, s.ctypes.data, fl.ctypes.data,
                                     ctypes.byref(ns)) == fa.OK
    assert ns.value == 4 and o[4:].tolist() == [-1] * 3 and s[4:].tolist() == [INF] * 3 and fl.sum() == 4


@pytest.mark.parametrize("D,f,says", [(3, 1, "f = 1"), (6, 1, "f = 1"), (10, 2, "f = 2"), (5, -1, "f = -1"),
                                      (2, 0, "f = 0"), (129, 0, "at most 128"), (0, 0, "D")])
def test_fa_bulyan_select_refuses_bad_f(fa, D, f, says):
    Q = np.zeros((max(D, 1), max(D, 1)), F64)
    rc = fa.lib().fa_bulyan_select(Q.ctypes.data, D, f, None, None, None, None)
    assert rc == fa.ERR_ARG and says in fa.last_error(), fa.last_error()


def test_fa_bulyan_select_null_and_optional_pointers(fa):
    assert fa.lib().fa_bulyan_select(None, 3, 0, None, None, None, None) == fa.ERR_ARG and "dist" in fa.last_error()
    Q = sym([[0, 25, 0], [25, 0, 25], [0, 25, 0]])
    ns = ctypes.c_int(-1)
    assert fa.lib().fa_bulyan_select(Q.ctypes.data, 3, 0, None, None, None, ctypes.byref(ns)) == fa.OK and ns.value == 3


# ------------------------------------------------------------------ the library, no device

def test_probe_without_a_device(fa):
    for in_dt, out_dt in ((fa.F32, fa.F32), (fa.F32, fa.BF16), (fa.BF16, fa.BF16), (fa.BF16, fa.F32), (fa.F16, fa.F16),
                          (fa.F16, fa.F32), (fa.F32, fa.F16)):
        for D, keep in ((1, 1), (5, 3), (128, 1), (128, 128)):
            fa.centered_device([None] * D, 0, in_dt, None, out_dt, keep=keep)  # n == 0: FA_OK, no device


def test_raw_entry_refusals_before_any_device_call(fa):
    buf = np.zeros(64, F32)
    a = buf.ctypes.data
    for D in (0, 129):
        with pytest.raises(fa.FaError) as e:
            fa.centered_device([None] * D, 0, fa.F32, None, fa.F32, keep=1)
        assert e.value.code == fa.ERR_ARG and "D" in str(e.value)
    for keep in (0, -1, 4):
        with pytest.raises(fa.FaError) as e:
            fa.centered_device([None] * 3, 0, fa.F32, None, fa.F32, keep=keep)
        assert e.value.code == fa.ERR_ARG and "keep %d" % keep in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.centered_device([None] * 3, 0, 3, None, fa.F32, keep=1)
    assert e.value.code == fa.ERR_ARG and "dtype" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.centered_device([None] * 3, 0, fa.BF16, None, fa.F16, keep=1)  # bf16 <-> f16
    assert e.value.code == fa.ERR_ARG
    with pytest.raises(fa.FaError) as e:
        fa.centered_device([a, None, a], 4, fa.F32, a, fa.F32, keep=1)
    assert e.value.code == fa.ERR_ARG and "client pointer 1" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.centered_device([a, a + 2, a], 4, fa.F32, a, fa.F32, keep=1)
    assert e.value.code == fa.ERR_ALIGN
    with pytest.raises(fa.FaError) as e:
        fa.centered_device([a, a, a], 4, fa.F32, None, fa.F32, keep=1)
    assert e.value.code == fa.ERR_ARG and "output" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.centered_device([a, a, a], 4, fa.F32, a + 2, fa.F32, keep=1)
    assert e.value.code == fa.ERR_ALIGN


def test_stage_entries_need_a_context(fa):
    L = fa.lib()
    assert L.fa_set_bulyan(None, -1, 1) == fa.ERR_ARG and "ctx" in fa.last_error()
    assert L.fa_set_bulyan(None, -1, -2) == fa.ERR_ARG and "f = -2" in fa.last_error()  # before anything else
    assert L.fa_bulyan_get_round(None, 1, None, None, None, None, None) == fa.ERR_ARG


# ------------------------------------------------------------------ the drop-in's flags

def aggregator_bin():
    from conftest import PKG_DIR
    agg = os.path.join(PKG_DIR, "bin", "fa_aggregator")
    assert os.access(agg, os.X_OK), "build the package first"
    return agg


@pytest.mark.parametrize("args,says", [
    (["--mode", "bulyan"], "--bulyan-f"),                                   # the mode without its f
    (["--bulyan-f", "1"], "--mode bulyan"),                                 # f without the mode
    (["--mode", "trimmed", "--bulyan-f", "1"], "--mode bulyan"),
    (["--mode", "bulyan", "--bulyan-f", "1", "--layout", "rs"], "--layout rs"),
    (["--mode", "bulyan", "--bulyan-f", "1", "--clip-norm", "1"], "--clip-norm"),
    (["--mode", "bulyan", "--bulyan-f", "1", "--krum-f", "1"], "--krum-f"),
    (["--mode", "bulyan", "--bulyan-f", "1", "--trim", "1"], "--trim"),
    (["--mode", "bulyan", "--bulyan-f", "-1"], "--bulyan-f -1"),
    (["--mode", "bulyan", "--bulyan-f", "2"], "--bulyan-f 2"),              # 4F + 3 = 11 > 7
])
def test_aggregator_flag_refusals_exit_2(args, says):
    """Refused while the arguments are parsed: usage on stderr, exit 2, before any device or socket is opened."""
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "7"] + args, capture_output=True, text=True,
                       timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "usage: fa_aggregator" in r.stderr and "[--bulyan-f F]" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""


def test_aggregator_refuses_more_than_128_owners():
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "129", "--mode", "bulyan", "--bulyan-f", "1"],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 2 and "128" in r.stderr
