"""CPU: the geomed stage (fa.h "Geomed stage") without a device -- fa_geomed_weights against the numpy helper
(tests/geomed_ref.py) bit for bit, the no-device probe and the refusals of the library, and the helper itself on two
attacks: what the rule is for."""
import ctypes
import math

import numpy as np
import pytest

import geomed_ref as G

F32, F64 = np.float32, np.float64
INF, NAN = math.inf, math.nan


def bits32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32).tolist()


def check_weights(fa, w, Q, inc, nu):
    got, ginc = fa.geomed_weights(w, Q, inc, nu)
    exp, einc, _ = G.weights(w, Q, inc, nu)
    assert bits32(got) == bits32(exp), (w, Q, inc, nu, got, exp)
    assert ginc.tolist() == einc.tolist(), (w, Q, inc, nu, ginc, einc)
    return got, ginc


# ------------------------------------------------------------------ fa_geomed_weights

@pytest.mark.parametrize("D", [1, 2, 3, 8, 33, 128])
def test_weights_on_random_distances(fa, O, D):
    rng = np.random.default_rng(0x6E0 + D)
    for case in range(40):
        w = O.weights(D) if case % 2 else rng.uniform(0.01, 3.0, D).astype(F32)
        Q = 10.0 ** rng.uniform(-12, 12, D)
        inc = rng.random(D) < 0.9 if case % 3 == 0 else np.ones(D, bool)
        got, ginc = check_weights(fa, w, Q, inc, 10.0 ** rng.uniform(-8, 0))
        if ginc.any():  # the mass of everyone who entered is kept
            assert abs(float(got.astype(F64).sum()) - float(w.astype(F64).sum())) < 1e-5 * float(w.astype(F64).sum())


def test_weights_below_the_floor_are_the_plain_weights_rescaled(fa):
    w = np.asarray([0.25, 0.25, 0.5], F32)
    # every N_k <= nu: beta_k = w_k / nu, B = W / nu, alpha = w up to the roundings of rule 4
    got, _ = check_weights(fa, w, [1e-14, 0.0, 1e-16], np.ones(3, bool), 1e-6)
    assert np.allclose(got, w, rtol=1e-6)
    got, _ = check_weights(fa, w, [0.0, 0.0, 0.0], np.ones(3, bool), 1e-6)  # Q = 0 for everyone
    assert np.allclose(got, w, rtol=1e-6)
    got, _ = check_weights(fa, w, [4.0, 0.0, 1.0], np.ones(3, bool), 0.5)  # N = 2, 0 -> nu, 1
    assert np.allclose(got, np.asarray([0.125, 0.5, 0.5]) / 1.125, rtol=1e-6)


def test_nan_and_inf_distances_exclude(fa):
    w = np.asarray([0.25, 0.25, 0.25, 0.25], F32)
    got, inc = check_weights(fa, w, [1.0, NAN, INF, 4.0], np.ones(4, bool), 1e-6)
    assert inc.tolist() == [True, False, False, True] and got[1] == 0 and got[2] == 0
    assert np.allclose(got[[0, 3]], [2 / 3, 1 / 3], rtol=1e-6)  # W = 1 stays: the excluded owners' mass moves
    got, inc = check_weights(fa, w, [1.0, -1.0, 1.0, 1.0], np.ones(4, bool), 1e-6)  # sqrt of a negative: NaN
    assert inc.tolist() == [True, False, True, True]


def test_zero_negative_and_nan_weights_are_excluded(fa):
    w = np.asarray([0.5, 0.0, -0.25, NAN, 0.5], F32)
    got, inc = check_weights(fa, w, [1.0, 1.0, 1.0, 1.0, 1.0], np.ones(5, bool), 1e-6)
    assert inc.tolist() == [True, False, False, False, True] and bits32(got) == bits32([0.5, 0, 0, 0, 0.5])


def test_everyone_excluded_and_overflow_fall_back(fa):
    w = np.asarray([0.5, 0.5], F32)
    got, inc = check_weights(fa, w, [NAN, INF], np.ones(2, bool), 1e-6)
    assert not inc.any() and bits32(got) == [0, 0]  # B = 0 is not > 0: alpha = w, for nobody
    got, inc = check_weights(fa, w, [1.0, 1.0], np.zeros(2, bool), 1e-6)
    assert not inc.any() and bits32(got) == [0, 0]
    # W / B overflows: beta = w / N is tiny against W
    big = np.asarray([3e38, 3e38], F32)
    got, inc = check_weights(fa, big, [1e300, 1e300], np.ones(2, bool), 1e-6)
    assert inc.all() and np.isfinite(got).all()
    tiny = np.asarray([1e-45, 1.0], F32)
    got, inc = check_weights(fa, tiny, [1e308, 1e308], np.ones(2, bool), 1e-6)
    assert inc.all()
    # the largest beta fp32 inputs can make (3e38 over the smallest subnormal floor) is far from overflowing fp64
    got, inc = check_weights(fa, np.asarray([3e38, 3e38], F32), [0.0, 1.0], np.ones(2, bool), 1e-45)
    assert inc.all() and got[0] == np.inf and got[1] < 1e-6  # nearly all of W = 6e38 lands on one owner: past fp32


def test_weights_refusals(fa):
    L = fa.lib()
    w, q, inc, out = np.ones(3, F32), np.ones(3, F64), np.ones(3, np.intc), np.ones(3, F32)
    args = (w.ctypes.data, q.ctypes.data, inc.ctypes.data)
    assert L.fa_geomed_weights(None, q.ctypes.data, inc.ctypes.data, 3, 1e-6, out.ctypes.data) == fa.ERR_ARG
    assert L.fa_geomed_weights(*args, 0, 1e-6, out.ctypes.data) == fa.ERR_ARG and "D" in fa.last_error()
    for nu in (0.0, -1.0, INF, NAN):
        assert L.fa_geomed_weights(*args, 3, nu, out.ctypes.data) == fa.ERR_ARG and "nu" in fa.last_error()
    assert L.fa_geomed_weights(*args, 3, 1e-6, out.ctypes.data) == fa.OK


# ------------------------------------------------------------------ the library, no device

def test_abi_version_stays_7(fa):
    assert fa.lib().fa_version() == 7
    assert fa.GEOMED_MAX_CLIENTS == 128 and fa.GEOMED_MAX_ITERS == 64


def test_probe_without_a_device(fa):
    for dt in (fa.F32, fa.BF16, fa.F16):
        for D in (1, 5, 128):
            q, b = fa.geomed_pass_device([None] * D, np.ones(D, F32), 0, dt)  # n == 0: FA_OK, zeros
            assert q.dtype == F64 and q.view(np.uint64).tolist() == [0] * D and b.view(np.uint64).tolist() == [0] * D


def test_raw_entry_refusals_before_any_device_call(fa):
    buf = np.zeros(64, F32)
    a = buf.ctypes.data
    for D in (0, 129):
        with pytest.raises(fa.FaError) as e:
            fa.geomed_pass_device([None] * D, np.ones(D, F32), 0, fa.F32)
        assert e.value.code == fa.ERR_ARG and "D" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.geomed_pass_device([None] * 3, np.ones(3, F32), 0, 3)
    assert e.value.code == fa.ERR_ARG and "dtype" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.geomed_pass_device([a, None, a], np.ones(3, F32), 4, fa.F32)
    assert e.value.code == fa.ERR_ARG and "client pointer 1" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.geomed_pass_device([a, a + 2, a], np.ones(3, F32), 4, fa.F32)
    assert e.value.code == fa.ERR_ALIGN
    with pytest.raises(fa.FaError) as e:
        fa.geomed_pass_device([a, a, a], np.ones(3, F32), 4, fa.F32, v=a + 2)
    assert e.value.code == fa.ERR_ALIGN and "d_v" in str(e.value)
    L = fa.lib()
    arr = (ctypes.c_void_p * 3)(a, a, a)
    w = np.ones(3, F32)
    out = np.ones(3, F64)
    assert L.fa_geomed_pass_device(None, 0, arr, None, 3, 0, fa.F32, None, out.ctypes.data, out.ctypes.data, None) == fa.ERR_ARG
    assert "h_weights" in fa.last_error()
    assert L.fa_geomed_pass_device(None, 0, arr, w.ctypes.data, 3, 0, fa.F32, None, None, out.ctypes.data, None) == fa.ERR_ARG
    assert "h_sumsq" in fa.last_error()
    assert L.fa_geomed_pass_device(None, 0, arr, w.ctypes.data, 3, 4, fa.F32, None, out.ctypes.data, None, None) == fa.ERR_ARG
    assert "h_nonfinite" in fa.last_error()


def test_stage_entries_check_their_numbers_before_the_context(fa):
    L = fa.lib()
    assert L.fa_set_geomed(None, -1, 4, 1e-6) == fa.ERR_ARG and "ctx" in fa.last_error()
    for iters in (-1, 65):
        assert L.fa_set_geomed(None, -1, iters, 1e-6) == fa.ERR_ARG and "iters = %d" % iters in fa.last_error()
    for nu in (0.0, -1e-6, INF, NAN):
        assert L.fa_set_geomed(None, -1, 4, nu) == fa.ERR_ARG and "nu" in fa.last_error()
    assert L.fa_set_geomed(None, -1, 0, 0.0) == fa.ERR_ARG and "ctx" in fa.last_error()  # removing needs no nu
    assert L.fa_geomed_get_round(None, 1, None, None, None, None, None) == fa.ERR_ARG
    assert L.fa_get_geomed(None, -1, None, None) == fa.ERR_ARG


# ------------------------------------------------------------------ the rule on two attacks (the helper alone)

ATTACK_N, ATTACK_T = 4099, 8


def attack(D, bad, how, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, ATTACK_N).astype(F32)
    xs = []
    for k in range(D):
        if k < bad:
            xs.append((g + F32(100.0)).astype(F32) if how == "shift" else (F32(-100.0) * g).astype(F32))
        else:
            xs.append((g + F32(0.1) * rng.uniform(-1, 1, ATTACK_N).astype(F32)).astype(F32))
    honest = np.mean(np.asarray(xs[bad:], F64), axis=0)
    return xs, honest


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, F64) - b) ** 2)))


@pytest.fixture(scope="module")
def attack_rounds(O):
    out = {}
    for D, bad, how in ((11, 3, "shift"), (8, 2, "scale")):
        xs, honest = attack(D, bad, how, 0xA77 + D)
        w = np.full(D, 1.0 / D, F32)
        out[how] = (xs, honest, w, G.geomed_round(O, xs, "f32", w, ATTACK_T, 1e-6))
    return out


@pytest.mark.parametrize("how", ["shift", "scale"])
def test_the_aggregate_stays_with_the_honest_owners(O, attack_rounds, how):
    xs, honest, w, r = attack_rounds[how]
    plain = rms(O.fedavg(xs, w), honest)
    robust = rms(r["aggregate"], honest)
    print("%s: plain FedAvg %.4g, geometric median %.4g from the honest mean (rms)" % (how, plain, robust))
    assert r["passes"] == ATTACK_T and r["included"].all()  # nobody is discarded, only down-weighted
    assert robust < plain / 100, (how, robust, plain)


@pytest.mark.parametrize("how", ["shift", "scale"])
def test_the_objective_does_not_increase(attack_rounds, how):
    obj = attack_rounds[how][3]["objective"]
    assert len(obj) == ATTACK_T and all(obj[t + 1] <= obj[t] for t in range(ATTACK_T - 1)), obj


def test_a_nan_bucket_voids_the_first_pass_once(O):
    rng = np.random.default_rng(3)
    xs = [rng.uniform(-1, 1, 67).astype(F32) for _ in range(5)]
    xs[2][5] = NAN
    w = np.asarray([0.2, 0.2, 0.2, 0.0, 0.4], F32)
    r = G.geomed_round(O, xs, "f32", w, 3, 1e-6)
    assert r["voided"] == 1 and r["passes"] == 3 and r["included"].tolist() == [True, True, False, False, True]
    assert np.isfinite(r["aggregate"]).all() and r["weights"].shape == (4, 5) and (r["weights"][:, [2, 3]] == 0).all()
    G.assert_bits(r["aggregate"], G.check_trace(O, xs, "f32", w, 1e-6, (r["sumsq"], r["weights"], r["included"], r["objective"]),
                                                "the helper's own trace"), "rule 5")
