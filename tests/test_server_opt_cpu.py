"""CPU: the server-optimizer reference helper (tests/server_opt_ref.py) and what libfa.so and the drop-in
answer without a device.

The helper is checked on hand-written columns with the expected bits written out and against a float64
evaluation of the same formulas; the library through its constants, fa_version, the no-device probe
(fa_server_opt_device with n == 0) and its refusals; the drop-in through its parse-time refusals.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import server_opt_ref as S

F32 = np.float32


def one(v):
    return np.array([v], np.uint32).view(F32) if isinstance(v, (int, np.integer)) else np.array([v], F32)


def bits(a):
    return int(np.ascontiguousarray(a, F32).view(np.uint32)[0])


# ------------------------------------------------------------------ the helper

HP = dict(lr=1.0, beta1=0.5, beta2=0.75, tau=1.0)


def test_adam_from_zero_state():
    x, m, v = S.step(S.ADAM, one(3.0), one(1.0), one(0.0), one(0.0), **HP)
    assert (bits(x), bits(m), bits(v)) == (bits(one(1.5)), bits(one(1.0)), bits(one(1.0)))


@pytest.mark.parametrize("v0,v1,x1", [
    (16.0, 15.0, 0x3F9A446C),  # s = 16 - 4 > 0: v' = v - u
    (1.0, 2.0, 0x3FB504F3),    # s = 1 - 4 < 0: v' = v + u
    (4.0, 4.0, 0x3FAAAAAB),    # s == 0: v' = v
])
def test_yogi_three_signs(v0, v1, x1):
    x, m, v = S.step(S.YOGI, one(3.0), one(1.0), one(0.0), one(v0), **HP)
    assert bits(v) == bits(one(v1)) and bits(m) == bits(one(1.0))
    assert bits(x) == x1, hex(bits(x))


def test_momentum_column():
    x, m, v = S.step(S.MOMENTUM, one(3.0), one(1.0), one(0.5), None, lr=1.0, beta1=0.5)
    assert v is None and bits(m) == bits(one(2.25)) and bits(x) == bits(one(3.25))


def test_adagrad_column():
    # d = 2, m' = .5*0 + .5*2 = 1, v' = 5 + 4 = 9, x' = 1 + 1 / (3 + 1) = 1.25
    x, m, v = S.step(S.ADAGRAD, one(3.0), one(1.0), one(0.0), one(5.0), **HP)
    assert (bits(x), bits(m), bits(v)) == (bits(one(1.25)), bits(one(1.0)), bits(one(9.0)))


@pytest.mark.parametrize("rule", S.RULES)
def test_aggregate_equal_to_x_with_zero_state_leaves_x(rule):
    x0 = np.array([0.375, -2.5, 1e-40, 3e38], F32)
    z = np.zeros(4, F32)
    x, m, v = S.step(rule, x0, x0, z, None if rule == S.MOMENTUM else z, lr=0.1)
    assert np.array_equal(x.view(np.uint32), x0.view(np.uint32))
    assert not m.any() and (v is None or not v.any())


@pytest.mark.parametrize("rule", S.RULES)
def test_nan_aggregate_poisons_the_state(rule):
    x, m, v = S.step(rule, one(np.nan), one(1.0), one(0.25), None if rule == S.MOMENTUM else one(2.0), lr=0.1)
    assert np.isnan(x[0]) and np.isnan(m[0]) and (v is None or np.isnan(v[0]))


def test_yogi_nan_when_v_minus_q_is_nan():
    # v = q = inf: s = inf - inf = NaN -> v' is a quiet NaN
    x, m, v = S.step(S.YOGI, one(np.inf), one(1.0), one(0.0), one(np.inf), **HP)
    assert np.isnan(v[0]) and np.isnan(x[0])


def test_bootstrap():
    a = np.array([1.5, -0.0, np.inf], F32)
    x, m, v = S.bootstrap(S.ADAM, a)
    assert np.array_equal(x.view(np.uint32), a.view(np.uint32)) and not m.any() and not v.any()
    assert not np.signbit(m).any() and not np.signbit(v).any()
    assert S.bootstrap(S.MOMENTUM, a)[2] is None


def test_16_bit_outputs():
    # fp16: beyond 65504 rounds to inf; the largest value that still rounds down stays finite
    r = S.round_out(np.array([65519.0, 65520.0, -70000.0, 6e-8], F32), "f16")
    assert r[0] == np.float16(65504.0) and np.isposinf(r[1]) and np.isneginf(r[2])
    assert r.view(np.uint16)[3] == 0x0001  # an fp16 subnormal, not flushed
    # bf16: ties go to even -- 1 + 2^-8 is half way between 0x3F80 and 0x3F81, 1 + 3 * 2^-8 between 0x3F81 and 0x3F82
    b = S.round_out(np.array([1.00390625, 1.01171875, 1.0039063692092896], F32), "bf16")
    assert list(b) == [0x3F80, 0x3F82, 0x3F81]
    # through a step: x' = 65504 + 1 * 32 / (0 + 1)... momentum with lr 1: m' = d, x' = avg
    x, _, _ = S.step(S.MOMENTUM, one(65536.0), one(65504.0), one(0.0), None, lr=1.0, beta1=0.0)
    assert np.isposinf(S.round_out(x, "f16")[0])


@pytest.mark.parametrize("rule", S.RULES)
def test_helper_against_float64(rule):
    """Three steps on random data: the fp32 helper stays within a few fp32 ulps per step of the float64
    evaluation (restarted from the fp32 state each step, so the bound is per step).  Each rule is at most a
    dozen roundings deep; every intermediate is bounded by a small multiple of the result's scale here (x in
    [-1, 1), |d| <= 2.1, the step |lr m / (sqrt v + tau)| <= 0.1 * 2.1 / 0.5), so 16 ulps of max(|x'|, 1),
    of max(|m'|, 1) and of max(v', 1) cover the accumulated relative error with room."""
    rng = np.random.default_rng(100 + rule)
    n = 4099
    x = rng.uniform(-1, 1, n).astype(F32)
    m = (rng.standard_normal(n) * 0.05).astype(F32)
    v = rng.uniform(0.25, 1.0, n).astype(F32)
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    ulp = float(np.finfo(F32).eps)
    for _ in range(3):
        avg = (x + rng.standard_normal(n).astype(F32) * F32(0.1)).astype(F32)
        gx, gm, gv = S.step(rule, avg, x, m, v, **hp)
        rx, rm, rv = S.step64(rule, avg, x, m, v, **hp)
        assert np.all(np.abs(gx - rx) <= 16 * ulp * np.maximum(np.abs(rx), 1))
        assert np.all(np.abs(gm - rm) <= 16 * ulp * np.maximum(np.abs(rm), 1))
        if rule != S.MOMENTUM:
            assert np.all(np.abs(gv - rv) <= 16 * ulp * np.maximum(np.abs(rv), 1))
            v = gv
        x, m = gx, gm
        assert np.isfinite(x).all()


def test_fused_variant_differs_from_the_second_step_on():
    """Why the GPU parity tests run three steps: a variant that fuses beta m + c d and beta v + c q (what a
    contracting compiler makes of them) agrees on the first step after m = v = 0 and not afterwards."""
    rng = np.random.default_rng(7)
    n = 4099
    b1, b2, lr, tau = F32(0.9), F32(0.99), F32(0.1), F32(1e-3)
    c1, c2 = F32(F32(1) - b1), F32(F32(1) - b2)

    def fused(avg, x, m, v):
        d = (avg - x).astype(F32)
        m1 = (np.float64(b1) * m + np.float64(c1) * d).astype(F32)   # one rounding where the rule has three
        q = (d * d).astype(F32)
        v1 = (np.float64(b2) * v + np.float64(c2) * q).astype(F32)
        return (x + ((lr * m1).astype(F32) / (np.sqrt(v1).astype(F32) + tau).astype(F32)).astype(F32)).astype(F32), m1, v1

    x = rng.uniform(-1, 1, n).astype(F32)
    xs, ms, vs = x, np.zeros(n, F32), np.zeros(n, F32)
    xf, mf, vf = x, np.zeros(n, F32), np.zeros(n, F32)
    diffs = []
    for _ in range(3):
        avg = (x + rng.standard_normal(n).astype(F32) * F32(0.1)).astype(F32)
        xs, ms, vs = S.step(S.ADAM, avg, xs, ms, vs, lr, b1, b2, tau)
        xf, mf, vf = fused(avg, xf, mf, vf)
        diffs.append(int(np.count_nonzero(ms.view(np.uint32) != mf.view(np.uint32)) +
                         np.count_nonzero(vs.view(np.uint32) != vf.view(np.uint32))))
    assert diffs[0] == 0 and diffs[1] > 0 and diffs[2] > 0, diffs


# ------------------------------------------------------------------ the library, no device

def test_constants(fa):
    assert (fa.OPT_NONE, fa.OPT_MOMENTUM, fa.OPT_ADAGRAD, fa.OPT_ADAM, fa.OPT_YOGI) == (0, 1, 2, 3, 4)
    assert (S.NONE, S.MOMENTUM, S.ADAGRAD, S.ADAM, S.YOGI) == (0, 1, 2, 3, 4)


def test_abi_version_stays_7(fa):
    assert fa.lib().fa_version() == 7


@pytest.mark.parametrize("rule", S.RULES)
def test_probe_without_a_device(fa, rule):
    for out_dtype in (fa.F32, fa.BF16, fa.F16):
        fa.server_opt_device(None, None, None, None, 0, None, out_dtype, rule=rule, lr=0.1)  # n == 0: FA_OK


def test_probe_momentum_needs_no_v(fa):
    fa.server_opt_device(None, None, None, None, 0, None, fa.F32, rule=fa.OPT_MOMENTUM, lr=1.0, beta2=7.0, tau=-1.0)


@pytest.mark.parametrize("kw,field", [
    (dict(rule=5, lr=0.1), "rule"),
    (dict(rule=-1, lr=0.1), "rule"),
    (dict(rule=3, lr=float("nan")), "lr"),
    (dict(rule=3, lr=-1.0), "lr"),
    (dict(rule=1, lr=float("inf")), "lr"),
    (dict(rule=3, lr=0.1, beta1=1.0), "beta1"),
    (dict(rule=1, lr=0.1, beta1=-0.5), "beta1"),
    (dict(rule=3, lr=0.1, beta2=-0.1), "beta2"),
    (dict(rule=4, lr=0.1, beta2=1.0), "beta2"),
    (dict(rule=4, lr=0.1, tau=0.0), "tau"),
    (dict(rule=2, lr=0.1, tau=float("inf")), "tau"),
    (dict(rule=0, lr=0.1), "rule"),  # FA_OPT_NONE takes no step
])
def test_probe_refusals_name_the_field(fa, kw, field):
    with pytest.raises(fa.FaError) as e:
        fa.server_opt_device(None, None, None, None, 0, None, fa.F32, **kw)
    assert e.value.code == fa.ERR_ARG and field in str(e.value), str(e.value)


def test_probe_refuses_a_bad_out_dtype(fa):
    with pytest.raises(fa.FaError) as e:
        fa.server_opt_device(None, None, None, None, 0, None, 3, rule=fa.OPT_ADAM, lr=0.1)
    assert e.value.code == fa.ERR_ARG


def test_null_and_misaligned_pointers_are_refused_before_any_device_call(fa):
    buf = np.zeros(64, F32)
    a = buf.ctypes.data
    with pytest.raises(fa.FaError) as e:  # n > 0 with a null state pointer
        fa.server_opt_device(a, a, None, a, 4, None, fa.F32, rule=fa.OPT_ADAM, lr=0.1)
    assert e.value.code == fa.ERR_ARG and "d_m" in str(e.value)
    with pytest.raises(fa.FaError) as e:  # the adaptive rules need v
        fa.server_opt_device(a, a, a, None, 4, None, fa.F32, rule=fa.OPT_YOGI, lr=0.1)
    assert e.value.code == fa.ERR_ARG and "d_v" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.server_opt_device(a + 2, a, a, a, 4, None, fa.F32, rule=fa.OPT_ADAM, lr=0.1)
    assert e.value.code == fa.ERR_ALIGN
    with pytest.raises(fa.FaError) as e:
        fa.server_opt_device(a, a, a, a, 4, a + 1, fa.BF16, rule=fa.OPT_ADAM, lr=0.1)
    assert e.value.code == fa.ERR_ALIGN


# ------------------------------------------------------------------ the drop-in's flags

def aggregator_bin():
    from conftest import PKG_DIR
    agg = os.path.join(PKG_DIR, "bin", "fa_aggregator")
    assert os.access(agg, os.X_OK), "build the package first"
    return agg


@pytest.mark.parametrize("args,says", [
    (["--server-lr", "0.1"], "--server-opt"),                                       # --server-* without its rule
    (["--server-beta1", "0.5"], "--server-opt"),
    (["--server-state", "/nonexistent/state"], "--server-opt"),
    (["--server-opt", "adam"], "--server-lr"),                                      # the rule without its rate
    (["--server-opt", "sgd", "--server-lr", "0.1"], "--server-opt sgd"),
    (["--server-opt", "adam", "--server-lr", "0.1", "--mode", "literal"], "--mode literal"),
    (["--server-opt", "yogi", "--server-lr", "0.1", "--layout", "rs"], "--layout rs"),
    (["--server-opt", "adam", "--server-lr", "-1"], "--server-lr"),
    (["--server-opt", "adam", "--server-lr", "nan"], "--server-lr"),
    (["--server-opt", "momentum", "--server-lr", "1", "--server-beta1", "1.0"], "--server-beta1"),
    (["--server-opt", "adam", "--server-lr", "1", "--server-beta2", "-0.1"], "--server-beta2"),
    (["--server-opt", "adagrad", "--server-lr", "1", "--server-tau", "0"], "--server-tau"),
])
def test_aggregator_flag_refusals_exit_2(args, says):
    """Refused while the arguments are parsed: usage on stderr, exit 2, before any device or socket is opened."""
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "3"] + args, capture_output=True, text=True,
                       timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "usage: fa_aggregator" in r.stderr and "--server-opt momentum|adagrad|adam|yogi" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""


def state_file(path, magic=b"FASRVOPT", version=1, rule=3, parts=()):
    with open(path, "wb") as f:
        f.write(magic + struct.pack("<IIII", version, rule, len(parts), 0))
        for pid, n in parts:
            f.write(struct.pack("<iIQQ", pid, 0, n, 0) + np.zeros(3 * n, F32).tobytes())


@pytest.mark.parametrize("kw,says", [
    (dict(magic=b"FASRVOPX"), "magic"),
    (dict(version=2), "version"),
    (dict(rule=4), "rule"),  # written by --server-opt yogi, started with adam
])
def test_aggregator_refuses_a_foreign_state_file_exit_2(tmp_path, kw, says):
    path = str(tmp_path / "state.bin")
    state_file(path, parts=[(1, 5)], **kw)
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "3", "--server-opt", "adam", "--server-lr", "0.1",
                        "--server-state", path], capture_output=True, text=True, timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "--server-state" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""


def test_aggregator_refuses_a_truncated_state_file_exit_2(tmp_path):
    path = str(tmp_path / "state.bin")
    state_file(path, parts=[(1, 5)])
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 7)
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "3", "--server-opt", "adam", "--server-lr", "0.1",
                        "--server-state", path], capture_output=True, text=True, timeout=30)
    assert r.returncode == 2 and "listening" not in r.stderr, (r.returncode, r.stderr[-500:])
