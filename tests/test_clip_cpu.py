"""CPU: the clip stage's numpy helper (tests/clip_ref.py) on hand-written columns, fa_clip_scale against it, the
no-device probe and refusals of the library, and the drop-in's --clip-norm / --clip-state flags."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import clip_ref as R

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ the helper

def test_three_four_five():
    g = np.asarray([1.0, -2.0, 0.5], F32)
    x = (g + np.asarray([3.0, 4.0, 0.0], F32)).astype(F32)
    assert R.sumsq(x, g) == 25.0
    assert R.scale(25.0, 5.0) == (F32(1.0), True)   # N == C: not clipped
    assert R.scale(25.0, 2.5) == (F32(0.5), True)
    assert R.scale(0.0, 2.5) == (F32(1.0), True)


def test_nan_inf_and_huge_clients():
    g = np.zeros(4, F32)
    assert math.isnan(R.sumsq(np.asarray([1, np.nan, 0, 0], F32), g))
    assert R.sumsq(np.asarray([1, np.inf, 0, 0], F32), g) == math.inf
    assert math.isnan(R.sumsq(np.asarray([np.inf, 0, 0, 0], F32), np.asarray([np.inf, 0, 0, 0], F32)))  # inf - inf
    q = R.sumsq(np.full(4, 1e30, F32), g)
    assert q == 4 * float(F32(1e30)) ** 2 and math.isfinite(q)  # far beyond fp32, exact in fp64
    assert R.scale(float("nan"), 1.0) == (F32(0.0), False)
    assert R.scale(math.inf, 1.0) == (F32(0.0), False)
    s, inc = R.scale(q, 1.0)
    assert inc and s == F32(1.0 / math.sqrt(q)) and 0 < s < 1e-29


def test_the_difference_is_rounded_to_fp32_before_it_is_squared():
    g = np.asarray([1.0], F32)
    x = np.asarray([1e-10], F32)
    assert R.sumsq(x, g) == float(F32(F32(1e-10) - F32(1.0))) ** 2 == 1.0  # not (1 - 1e-10)^2


def test_weights_keep_the_mass_on_the_reference():
    w = np.asarray([0.25, 0.25, 0.5], F32)
    inc, wp, c0 = R.weights(w, np.asarray([1.0, 0.5, 0.0], F32), [True, True, False])
    assert inc == [0, 1] and wp.tolist() == [0.25, 0.125] and c0 == F32(0.625)
    inc, wp, c0 = R.weights(w, np.ones(3, F32), [True] * 3)
    assert inc == [0, 1, 2] and c0 == 0 and wp.tolist() == w.tolist()


def test_first_term_has_no_negative_zero():
    t = R.first_term(F32(0.5), np.asarray([-0.0, 0.0, -2.0, np.inf], F32))
    assert t.view(np.uint32).tolist() == np.asarray([0.0, 0.0, -1.0, np.inf], F32).view(np.uint32).tolist()


def test_aggregate_is_the_chain_with_the_reference_first(O):
    rng = np.random.default_rng(3)
    n, D = 67, 3
    g = rng.uniform(-1, 1, n).astype(F32)
    xs = [(g + rng.standard_normal(n).astype(F32) * F32(s)).astype(F32) for s in (0.01, 1.0, 0.01)]
    w = O.weights(D)
    C = 0.5
    Q, scales, included, n_clipped, a = R.clip_round(O, xs, "f32", w, g, C)
    assert n_clipped == 1 and included.all() and scales[1] < 1 and scales[0] == 1 and scales[2] == 1
    _, wp, c0 = R.weights(w, scales, included)
    acc = np.zeros(n, F64)
    acc = (F64(c0) * g.astype(F64) + acc).astype(F32)  # fma: the product is exact in fp64, rounded once
    for k in range(D):
        acc = (F64(wp[k]) * xs[k].astype(F64) + acc.astype(F64)).astype(F32)
    # fp64 evaluates each fma exactly enough: a 24 x 24-bit product plus a 24-bit addend can round differently
    # from a true fma only in double-rounding cases, so this is a cross-check to within 1 ulp, not a bit check
    assert np.all(np.abs(a - acc) <= np.spacing(np.abs(acc)))
    # an unclipped round is the plain chain, bit for bit
    _, s1, i1, n1, a1 = R.clip_round(O, xs, "f32", w, g, 1e30)
    assert n1 == 0 and a1.view(np.uint32).tolist() == O.fedavg(xs, w).view(np.uint32).tolist()


# ------------------------------------------------------------------ the library, no device

def test_abi_version_stays_7(fa):
    assert fa.lib().fa_version() == 7


def test_fa_clip_scale_is_the_helper(fa):
    rng = np.random.default_rng(11)
    qs = [25.0, 0.0, 6.25, float("nan"), math.inf, -1.0, 4e60, 5e-324, 1e-300, 1.7e308]
    qs += (10.0 ** rng.uniform(-12, 12, 1000)).tolist()
    for C in (5.0, 2.5, 1e-3, 3e38):
        for q in qs:
            s, ex = fa.clip_scale(q, C)
            rs, inc = R.scale(q, C)
            assert ex == (not inc) and s.view(np.uint32) == rs.view(np.uint32), (q, C, s, rs)


def test_probe_without_a_device(fa):
    for dt in (fa.F32, fa.BF16, fa.F16):
        q = fa.clip_sumsq_device([None] * 5, 0, dt, None)  # n == 0: FA_OK, zeros
        assert q.dtype == F64 and q.tolist() == [0.0] * 5


def test_raw_entry_refusals_before_any_device_call(fa):
    buf = np.zeros(64, F32)
    a = buf.ctypes.data
    with pytest.raises(fa.FaError) as e:
        fa.clip_sumsq_device([], 0, fa.F32, None)
    assert e.value.code == fa.ERR_ARG and "D" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.clip_sumsq_device([None], 0, 3, None)
    assert e.value.code == fa.ERR_ARG and "dtype" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.clip_sumsq_device([a, None], 4, fa.F32, a)
    assert e.value.code == fa.ERR_ARG and "client pointer 1" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.clip_sumsq_device([a, a], 4, fa.F32, None)
    assert e.value.code == fa.ERR_ARG and "d_ref" in str(e.value)
    with pytest.raises(fa.FaError) as e:
        fa.clip_sumsq_device([a, a + 2], 4, fa.F32, a)
    assert e.value.code == fa.ERR_ALIGN
    with pytest.raises(fa.FaError) as e:
        fa.clip_sumsq_device([a + 2], 4, fa.BF16, a + 2)
    assert e.value.code == fa.ERR_ALIGN and "reference" in str(e.value)
    import ctypes
    arr = (ctypes.c_void_p * 1)(a)
    assert fa.lib().fa_clip_sumsq_device(None, 0, arr, 1, 4, fa.F32, a, None, None) == fa.ERR_ARG  # h_sumsq is null
    assert "h_sumsq" in fa.last_error()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -1.0])
def test_set_clip_refuses_a_bad_bound_before_anything_else(fa, bad):
    assert fa.lib().fa_set_clip(None, -1, bad) == fa.ERR_ARG
    assert "max_norm" in fa.last_error()


def test_stage_entries_need_a_context(fa):
    L = fa.lib()
    assert L.fa_set_clip(None, -1, 1.0) == fa.ERR_ARG and "ctx" in fa.last_error()
    assert L.fa_clip_set_reference(None, 1, None) == fa.ERR_ARG
    assert L.fa_clip_get_reference(None, 1, None) == fa.ERR_ARG
    assert L.fa_clip_get_round(None, 1, None, None, None, None) == fa.ERR_ARG


# ------------------------------------------------------------------ the drop-in's flags

def aggregator_bin():
    from conftest import PKG_DIR
    agg = os.path.join(PKG_DIR, "bin", "fa_aggregator")
    assert os.access(agg, os.X_OK), "build the package first"
    return agg


@pytest.mark.parametrize("args,says", [
    (["--clip-norm", "1", "--mode", "literal"], "--mode literal"),
    (["--clip-norm", "1", "--mode", "trimmed"], "--mode trimmed"),
    (["--clip-norm", "1", "--mode", "median"], "--mode median"),
    (["--clip-norm", "1", "--layout", "rs"], "--layout rs"),
    (["--clip-norm", "0"], "--clip-norm 0"),
    (["--clip-norm", "-2"], "--clip-norm -2"),
    (["--clip-norm", "nan"], "--clip-norm"),
    (["--clip-norm", "inf"], "--clip-norm"),
    (["--clip-state", "/nonexistent/state"], "--clip-norm"),  # the file without its bound
])
def test_aggregator_flag_refusals_exit_2(args, says):
    """Refused while the arguments are parsed: usage on stderr, exit 2, before any device or socket is opened."""
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "3"] + args, capture_output=True, text=True,
                       timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "usage: fa_aggregator" in r.stderr and "--clip-norm C [--clip-state FILE]" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""


def clip_state_file(path, magic=b"FACLIPRF", version=1, parts=()):
    with open(path, "wb") as f:
        f.write(magic + struct.pack("<II", version, len(parts)))
        for pid, n in parts:
            f.write(struct.pack("<iIQ", pid, 0, n) + np.zeros(n, F32).tobytes())


@pytest.mark.parametrize("kw,says", [(dict(magic=b"FACLIPRX"), "magic"), (dict(magic=b"FASRVOPT"), "magic"),
                                     (dict(version=2), "version")])
def test_aggregator_refuses_a_foreign_clip_state_exit_2(tmp_path, kw, says):
    path = str(tmp_path / "clip.bin")
    clip_state_file(path, parts=[(1, 5)], **kw)
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "3", "--clip-norm", "1", "--clip-state", path],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "--clip-state" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""


def test_aggregator_refuses_a_truncated_clip_state_exit_2(tmp_path):
    path = str(tmp_path / "clip.bin")
    clip_state_file(path, parts=[(1, 5)])
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 3)
    r = subprocess.run([aggregator_bin(), "-i", "-1", "-c", "1", "-d", "3", "--clip-norm", "1", "--clip-state", path],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 2 and "listening" not in r.stderr, (r.returncode, r.stderr[-500:])
