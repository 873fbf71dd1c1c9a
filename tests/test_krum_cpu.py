"""CPU: the Krum stage's numpy helper (tests/krum_ref.py) on hand-written columns, fa_krum_select and
fa_krum_weights against it, the no-device probe and refusals of the library, and the drop-in's --krum-f /
--krum-m flags."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import krum_ref as K

F32, F64 = np.float32, np.float64
INF, NAN = math.inf, math.nan


def bits64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64).tolist()


def sym(rows):
    Q = np.asarray(rows, F64)
    assert Q.shape[0] == Q.shape[1] and bits64(Q) == bits64(Q.T)
    return Q


# ------------------------------------------------------------------ the helper

def test_three_four_five():
    x = np.asarray([1.0, -2.0, 0.5], F32)
    y = (x + np.asarray([3.0, 4.0, 0.0], F32)).astype(F32)
    assert K.pair_sumsq(x, y) == 25.0 and K.pair_sumsq(y, x) == 25.0
    Q = K.distances([x, y, x.copy()], "f32")
    assert Q.tolist() == [[0.0, 25.0, 0.0], [25.0, 0.0, 25.0], [0.0, 25.0, 0.0]]


def test_the_difference_is_rounded_to_fp32_before_it_is_squared():
    x = np.asarray([1.0], F32)
    y = np.asarray([1e-10], F32)
    assert K.pair_sumsq(x, y) == float(F32(F32(1.0) - F32(1e-10))) ** 2 == 1.0  # not (1 - 1e-10)^2


def test_nan_and_inf_propagate_and_the_diagonal_is_zero():
    a = np.asarray([1, NAN, 0, 0], F32)
    b = np.asarray([1, INF, 0, 0], F32)
    c = np.zeros(4, F32)
    Q = K.distances([a, b, c], "f32")
    assert math.isnan(Q[0, 1]) and math.isnan(Q[0, 2]) and Q[1, 2] == INF
    assert bits64(np.diag(Q)) == [0, 0, 0]  # +0, also for the bucket that holds a NaN
    assert math.isnan(K.pair_sumsq(b, b.copy()))  # inf - inf: why the diagonal is defined, not computed
    q = K.pair_sumsq(np.full(4, 1e30, F32), c)
    assert q == 4 * float(F32(1e30)) ** 2 and math.isfinite(q)  # far beyond fp32, exact in fp64


def test_nan_becomes_inf_in_the_scores():
    Q = sym([[0, 1, NAN, 2], [1, 0, 3, 4], [NAN, 3, 0, 5], [2, 4, 5, 0]])
    S = K.scores(Q, 0)  # D - f - 2 = 2 smallest of each row
    assert S.tolist() == [3.0, 4.0, 8.0, 6.0]
    Q = sym([[0, NAN, NAN, 2], [NAN, 0, 3, 4], [NAN, 3, 0, 5], [2, 4, 5, 0]])
    assert K.scores(Q, 0).tolist() == [INF, 7.0, 8.0, 6.0]


def test_the_tie_goes_to_the_lower_index():
    Q = sym([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]])
    S, sel = K.krum_select(Q, 0, 1)
    assert S.tolist() == [2.0] * 4 and sel.tolist() == [True, False, False, False]
    S, sel = K.krum_select(Q, 0, 3)
    assert sel.tolist() == [True, True, True, False]
    # two identical clients: Q = 0 between them, equal scores, the lower one wins
    Q = sym([[0, 9, 4, 4], [9, 0, 5, 5], [4, 5, 0, 0], [4, 5, 0, 0]])
    S, sel = K.krum_select(Q, 0, 1)
    assert S.tolist() == [8.0, 10.0, 4.0, 4.0] and sel.tolist() == [False, False, True, False]


def test_a_client_whose_row_is_all_inf_is_never_selected():
    Q = sym([[0, INF, INF, INF, INF], [INF, 0, 1, 2, 3], [INF, 1, 0, 1, 2], [INF, 2, 1, 0, 1], [INF, 3, 2, 1, 0]])
    S, sel = K.krum_select(Q, 0)  # m = D: the all-inf client still stays out
    assert S[0] == INF and np.isfinite(S[1:]).all() and sel.tolist() == [False, True, True, True, True]


def test_m_larger_than_the_finite_scores_selects_fewer():
    Q = np.full((5, 5), NAN)
    np.fill_diagonal(Q, 0.0)
    Q[3, 4] = Q[4, 3] = 1.0
    S, sel = K.krum_select(Q, 1, 4)  # D - f - 2 = 2 values each: every score holds an inf
    assert (S == INF).all() and not sel.any()
    Q[2, 3] = Q[3, 2] = 2.0
    Q[2, 4] = Q[4, 2] = 2.0
    S, sel = K.krum_select(Q, 1, 4)
    assert S.tolist() == [INF, INF, 4.0, 3.0, 3.0] and sel.tolist() == [False, False, True, True, True]


def test_weights_keep_the_round_mass():
    w = np.asarray([0.25, 0.25, 0.5], F32)
    assert K.weights(w, [True, True, True]).tolist() == w.tolist()
    assert K.weights(w, [True, True, False]).tolist() == [0.5, 0.5, 1.0]
    assert K.weights(w, [False, False, True]).tolist() == [0.5, 0.5, 1.0]
    assert K.weights(w, [False, False, False]).tolist() == w.tolist()          # W_s = 0: unchanged
    assert K.weights([0.0, 1.0, 1.0], [True, False, False]).tolist() == [0.0, 1.0, 1.0]  # W_s not > 0
    assert K.weights([INF, 1.0, 1.0], [False, True, True]).tolist() == [INF, 1.0, 1.0]  # W / W_s = inf


def test_aggregate_is_the_chain_over_the_selected(O):
    rng = np.random.default_rng(5)
    xs = [rng.uniform(-1, 1, 67).astype(F32) for _ in range(4)]
    w = O.weights(4)
    everyone = np.ones(4, bool)
    K.assert_bits(K.aggregate(O, xs, "f32", w, everyone), O.fedavg(xs, w), "nobody deselected: plain FedAvg")
    sel = np.asarray([True, False, True, True])
    wp = K.weights(w, sel)
    K.assert_bits(K.aggregate(O, xs, "f32", w, sel), O.fedavg([xs[0], xs[2], xs[3]], wp[[0, 2, 3]]), "three of four")
    assert K.aggregate(O, xs, "f32", w, np.zeros(4, bool)).view(np.uint32).tolist() == [0] * 67  # nobody: +0


# ------------------------------------------------------------------ the lattice inputs and their closed form

LATTICE_KINDS = ["f32", "bf16", "f16"]


def test_mian_chowla_is_a_sidon_sequence():
    c = K.mian_chowla(K.LATTICE_CLIENTS)
    assert c[:10] == [1, 2, 4, 8, 13, 21, 31, 45, 66, 81] and len(c) == 128 and c == sorted(set(c))
    sums = [c[a] + c[b] for a in range(128) for b in range(a, 128)]
    assert len(set(sums)) == len(sums)  # the Sidon property
    sq = [(c[a] - c[b]) ** 2 for a in range(128) for b in range(a + 1, 128)]
    assert len(set(sq)) == len(sq) == 8128  # so every entry of the matrix names its pair


@pytest.mark.parametrize("kind", LATTICE_KINDS)
def test_lattice_magnitudes_fit_their_formats(kind):
    n = K.LATTICE_N
    c, u, xs = K.lattice(n, kind)
    assert len(xs) == 128 and all(np.asarray(x).size == n for x in xs)
    assert sorted(set(u.tolist())) == [-2, -1, 1, 2]  # never 0: every element counts in every pair
    cu = int(np.abs(c).max()) * int(np.abs(u).max())
    assert cu < (2 ** 24 if kind == "f32" else 255)  # max |c_k u_i|: exact in the type
    span = int(c.max() - c.min()) * 2
    assert span < 2 ** 23  # max |(c_a - c_b) u_i|: exact in fp32, also in steps of its smallest subnormal
    assert span ** 2 * n < 2 ** 53  # any partial sum of any order is an exact integer
    assert K.lattice_distances(c, u).max() < 2.0 ** 53
    assert c.tolist() == (K.mian_chowla(128) if kind == "f32" else list(range(128)))
    for k in (0, 1, 77, 127):
        assert K.widen(xs[k], kind).astype(F64).tolist() == (c[k] * u).astype(F64).tolist()


@pytest.mark.parametrize("kind", LATTICE_KINDS)
def test_lattice_subnormal_inputs_are_subnormal(kind):
    c, u, xs = K.lattice(K.LATTICE_N, kind, K.SUBNORMAL_SCALE[kind])
    N = K.SMALLEST_NORMAL[kind]
    for k in range(128):
        w = np.abs(K.widen(xs[k], kind).astype(F64))
        assert w.tolist() == np.ldexp(np.abs(c[k] * u).astype(F64), K.pow2_exponent(K.SUBNORMAL_SCALE[kind])).tolist()
        if kind != "bf16" or k < 64:  # bf16: 2^-133 |c u| < 2^-126 needs |c u| < 128
            assert (w < N).all() and (w > 0).all() == (c[k] != 0)
        else:
            assert (w < 2 * N).all() and (w[np.abs(u) == 1] < N).all()
    # the fl32 differences: f32, all of them fp32 subnormals; bf16, those of clients at most 63 apart (16-bit
    # inputs widen to fp32 normals and subnormals alike; f16's are fp32 normals, its inputs f16 subnormals)
    if kind == "f32":
        assert int(c.max() - c.min()) * 2 * K.SUBNORMAL_SCALE[kind] < 2.0 ** -126
    if kind == "bf16":
        assert 63 * 2 * K.SUBNORMAL_SCALE[kind] < 2.0 ** -126 <= 64 * 2 * K.SUBNORMAL_SCALE[kind]


@pytest.mark.parametrize("kind", LATTICE_KINDS)
@pytest.mark.parametrize("D,n", [(5, K.LATTICE_N), (33, K.LATTICE_N), (128, 259)])
def test_lattice_closed_form_is_rule_1_bit_for_bit(kind, D, n):
    for scale in (1.0, K.SUBNORMAL_SCALE[kind]):
        c, u, xs = K.lattice(n, kind, scale)
        Q = K.lattice_distances(c, u, scale, D)
        assert Q.shape == (D, D) and (Q[np.triu_indices(D, 1)] > 0).all()
        assert bits64(Q) == bits64(K.distances(xs[:D], kind)), (kind, D, scale)
        if kind == "f32":
            assert len(set(Q[np.triu_indices(D, 1)].tolist())) == D * (D - 1) // 2


def test_lattice_closed_form_follows_a_prefix_of_u():
    c, u, xs = K.lattice(67, "bf16")
    for n in (1, 3, 8):
        assert bits64(K.lattice_distances(c, u[:n], 1.0, 9)) == bits64(K.distances([x[:n] for x in xs[:9]], "bf16"))


# ------------------------------------------------------------------ the library, no device

HAND = [
    ([[0, 1, NAN, 2], [1, 0, 3, 4], [NAN, 3, 0, 5], [2, 4, 5, 0]], 0),
    ([[0, NAN, NAN, 2], [NAN, 0, 3, 4], [NAN, 3, 0, 5], [2, 4, 5, 0]], 0),
    ([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]], 0),
    ([[0, 9, 4, 4], [9, 0, 5, 5], [4, 5, 0, 0], [4, 5, 0, 0]], 0),
    ([[0, INF, INF, INF, INF], [INF, 0, 1, 2, 3], [INF, 1, 0, 1, 2], [INF, 2, 1, 0, 1], [INF, 3, 2, 1, 0]], 0),
    ([[0, INF, INF, INF, INF], [INF, 0, 1, 2, 3], [INF, 1, 0, 1, 2], [INF, 2, 1, 0, 1], [INF, 3, 2, 1, 0]], 1),
    ([[0, NAN, NAN, NAN, NAN], [NAN, 0, NAN, NAN, NAN], [NAN, NAN, 0, 2, 2], [NAN, NAN, 2, 0, 1], [NAN, NAN, 2, 1, 0]], 1),
    ([[0, 25, 0], [25, 0, 25], [0, 25, 0]], 0),
]


def check_against_helper(fa, Q, f, m):
    S, sel = fa.krum_select(Q, f, m)
    rS, rsel = K.krum_select(Q, f, m)
    assert bits64(S) == bits64(rS), (Q.shape, f, m, S, rS)
    assert sel.tolist() == rsel.tolist(), (Q.shape, f, m, sel, rsel)
    return S, sel


def test_abi_version_stays_7(fa):
    assert fa.lib().fa_version() == 7


def test_fa_krum_select_is_the_helper_on_the_hand_written_matrices(fa):
    for rows, f in HAND:
        Q = sym(rows)
        D = Q.shape[0]
        for m in [None] + list(range(1, D - f + 1)):
            check_against_helper(fa, Q, f, m)


@pytest.mark.parametrize("D", [3, 4, 8, 33, 128])
def test_fa_krum_select_is_the_helper_on_random_matrices(fa, D):
    rng = np.random.default_rng(0xC0DE + D)
    fmax = (D - 3) // 2
    for case in range(60 if D <= 33 else 12):
        A = 10.0 ** rng.uniform(-6, 6, (D, D))
        if case % 3 == 1:  # few distinct values: many ties
            A = rng.integers(0, 4, (D, D)).astype(F64)
        Q = np.triu(A, 1)
        Q = Q + Q.T
        if case % 4 == 2:  # NaN / inf rows sprinkled in
            for k in rng.choice(D, max(1, D // 4), replace=False):
                Q[k, :] = Q[:, k] = rng.choice([NAN, INF])
            np.fill_diagonal(Q, 0.0)
        if case % 4 == 3:  # single NaN / inf entries
            for _ in range(D):
                a, b = rng.choice(D, 2, replace=False)
                Q[a, b] = Q[b, a] = rng.choice([NAN, INF])
        Q = sym(Q)
        f = int(rng.integers(0, fmax + 1))
        for m in (None, 1, int(rng.integers(1, D - f + 1))):
            check_against_helper(fa, Q, f, m)


def test_fa_krum_weights_is_the_helper(fa, O):
    rng = np.random.default_rng(17)
    for D in (3, 8, 33, 128):
        w = O.weights(D)
        got = fa.krum_weights(w, np.ones(D, bool))
        assert got.view(np.uint32).tolist() == w.view(np.uint32).tolist()  # all selected: unchanged to the bit
        for _ in range(40):
            sel = rng.random(D) < rng.uniform(0.1, 0.95)
            got, exp = fa.krum_weights(w, sel), K.weights(w, sel)
            assert got.view(np.uint32).tolist() == exp.view(np.uint32).tolist(), (D, sel)
            if sel.any() and not sel.all():
                assert abs(float(got[sel].astype(F64).sum()) - float(w.astype(F64).sum())) < 1e-5  # the mass is kept
    for w, sel in (([0.25, 0.25, 0.5], [0, 0, 0]), ([0.0, 1.0, 1.0], [1, 0, 0]), ([INF, 1.0, 1.0], [0, 1, 1]),
                   ([0.25, 0.25, 0.5], [1, 1, 0])):
        got, exp = fa.krum_weights(w, sel), K.weights(w, np.asarray(sel, bool))
        assert got.view(np.uint32).tolist() == exp.view(np.uint32).tolist(), (w, sel)


def test_probe_without_a_device(fa):
    for dt in (fa.F32, fa.BF16, fa.F16):
        for D in (1, 5, 128):
            q = fa.pairdist_device([None] * D, 0, dt)  # n == 0: FA_OK, D * D zeros
            assert q.dtype == F64 and q.shape == (D, D) and bits64(q) == [[0] * D] * D


def test_raw_entry_refusals_before_any_device_call(fa):
    buf = np.zeros(64, F32)
    a = buf.ctypes.data
    for D in (0, 129):
        with pytest.raises(fa.FaError) as e:
            fa.pairdist_device([None] * D, 0, fa.F32)
        assert e.value.code == fa.ERR_ARG and "D" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.pairdist_device([None] * 3, 0, 3)
    assert e.value.code == fa.ERR_ARG and "dtype" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.pairdist_device([a, None, a], 4, fa.F32)
    assert e.value.code == fa.ERR_ARG and "client pointer 1" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.pairdist_device([a, a + 2, a], 4, fa.F32)
    assert e.value.code == fa.ERR_ALIGN
    arr = (ctypes.c_void_p * 3)(a, a, a)
    assert fa.lib().fa_pairdist_device(None, 0, arr, 3, 4, fa.F32, None, None) == fa.ERR_ARG  # h_dist is null
    assert "h_dist" in fa.last_error()
    assert fa.lib().fa_pairdist_device(None, 0, arr, 3, 0, fa.F32, None, None) == fa.ERR_ARG  # also for the probe


@pytest.mark.parametrize("D,f,m,says", [(3, 1, 1, "f = 1"), (4, 1, 1, "f = 1"), (5, -1, 1, "f = -1"), (5, 2, 1, "f = 2"),
                                        (5, 1, 5, "m = 5"), (5, 1, 0, "m = 0"), (5, 1, -2, "m = -2"),
                                        (2, 0, 1, "f = 0"), (129, 0, 1, "at most 128"), (0, 0, 1, "D")])
def test_fa_krum_select_refuses_bad_f_and_m(fa, D, f, m, says):
    Q = np.zeros((max(D, 1), max(D, 1)), F64)
    rc = fa.lib().fa_krum_select(Q.ctypes.data, D, f, m, None, None, None)
    assert rc == fa.ERR_ARG and says in fa.last_error(), fa.last_error()


def test_fa_krum_select_null_and_optional_pointers(fa):
    assert fa.lib().fa_krum_select(None, 3, 0, 1, None, None, None) == fa.ERR_ARG and "dist" in fa.last_error()
    Q = sym([[0, 25, 0], [25, 0, 25], [0, 25, 0]])
    ns = ctypes.c_int(-1)
    assert fa.lib().fa_krum_select(Q.ctypes.data, 3, 0, -1, None, None, ctypes.byref(ns)) == fa.OK and ns.value == 3
    assert fa.lib().fa_krum_weights(None, None, 3, None) == fa.ERR_ARG


def test_stage_entries_need_a_context(fa):
    L = fa.lib()
    assert L.fa_set_krum(None, -1, 1, -1) == fa.ERR_ARG and "ctx" in fa.last_error()
    assert L.fa_set_krum(None, -1, -1, 1) == fa.ERR_ARG and "f = -1" in fa.last_error()  # before anything else
    assert L.fa_krum_get_round(None, 1, None, None, None, None) == fa.ERR_ARG


# ------------------------------------------------------------------ the drop-in's flags

def aggregator_bin():
    from conftest import PKG_DIR
    agg = os.path.join(PKG_DIR, "bin", "fa_aggregator")
    assert os.access(agg, os.X_OK), "build the package first"
    return agg


@pytest.mark.parametrize("args,says", [
    (["--krum-f", "1", "--clip-norm", "1"], "--clip-norm"),
    (["--krum-f", "1", "--mode", "literal"], "--mode literal"),
    (["--krum-f", "1", "--mode", "trimmed"], "--mode trimmed"),
    (["--krum-f", "1", "--mode", "median"], "--mode median"),
    (["--krum-f", "1", "--layout", "rs"], "--layout rs"),
    (["--krum-f", "-1"], "--krum-f -1"),
    (["--krum-f", "1", "--krum-m", "0"], "--krum-m 0"),
    (["--krum-m", "2"], "--krum-f"),  # m without f
])
def test_aggregator_flag_refusals_exit_2(args, says):
    """Refused while the arguments are parsed: usage on stderr, exit 2, before any device or socket is opened."""
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "5"] + args, capture_output=True, text=True,
                       timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "usage: fa_aggregator" in r.stderr and "--krum-f F [--krum-m M]" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""
