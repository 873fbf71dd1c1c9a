"""CPU: the secagg stage's host side (fa.h "Secagg stage") -- the known answer against tests/secagg_ref.py and
fa_secagg_mask_host, the owner's quantizer, the probe and the refusals that need no context.  The refusals that need a
part (its dtype, its other stages, an rs context, a reducing call without terms) are in test_secagg_stage_gpu.py: a
context needs a device.
"""
import ctypes

import numpy as np
import pytest

import secagg_ref as SA

U32 = np.uint32
KAT_KEY = np.frombuffer(bytes(range(32)), "<u4")
KAT_NONCE = np.asarray([0x09000000, 0x4A000000, 0], U32)
KAT_WORDS = [int(w, 16) for w in ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                                  "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]


def test_known_answer(fa):
    ref = SA.block_words(KAT_KEY, KAT_NONCE, [1])[0]
    assert [int(w) for w in ref] == KAT_WORDS
    assert ref.astype("<u4").tobytes()[:8] == bytes.fromhex("10f1e7e4d13b5915") and ref.astype("<u4").tobytes()[-4:] == bytes.fromhex("a2503c4e")
    assert [int(w) for w in fa.secagg_mask_host(KAT_KEY, KAT_NONCE, 16, 16)] == KAT_WORDS


@pytest.mark.parametrize("idx0", [0, 5, 2 ** 36 - 40])
def test_mask_host_equals_the_reference(fa, idx0):
    rng = np.random.default_rng(idx0 % 97)
    for n in (1, 15, 16, 40):
        key, nonce = rng.integers(0, 2 ** 32, 8, dtype=np.uint64), rng.integers(0, 2 ** 32, 3, dtype=np.uint64)
        got = fa.secagg_mask_host(key, nonce, idx0, n)
        assert got.dtype == U32 and np.array_equal(got, SA.mask(key, nonce, idx0, n)), (idx0, n)
    assert fa.secagg_mask_host(KAT_KEY, KAT_NONCE, idx0, 0).size == 0


def test_quantize_ties_saturation_and_nan(fa):
    v = np.asarray([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, 3e9, -3e9, np.inf, -np.inf, np.nan, 2147483520.0, -0.0], np.float32)
    codes, bad = fa.secagg_quantize(v, 1.0)
    top = 2 ** 31 - 1
    assert codes.tolist() == [0, 2, 2, 0, -2, 0, top, -top, top, -top, 0, 2147483520, 0] and bad == 1
    codes, bad = fa.secagg_quantize(np.asarray([0.1, -0.1, 1.0], np.float32), 65536.0)
    assert codes.tolist() == [round(float(np.float32(0.1)) * 65536), -round(float(np.float32(0.1)) * 65536), 65536] and bad == 0
    L = fa.lib()
    for q in (0.0, -1.0, float("nan"), float("inf")):
        assert L.fa_secagg_quantize(None, 0, q, None, None) == fa.ERR_ARG and "q" in fa.last_error()


def test_form_is_a_host_rule(fa):
    assert fa.secagg_form(3000, 0) == fa.SECAGG_TILE and fa.secagg_form(3000, 130) == fa.SECAGG_SPLIT
    assert fa.secagg_form(64 << 20, 130) == fa.SECAGG_TILE


def test_probe_and_refusals_without_a_context(fa):
    fa.secagg_unmask_device([0], 0, None, fa.BF16, scale=2.0 ** -16, idx0=2 ** 36)  # the probe: no device touched

    def refused(code, word, **kw):
        args = dict(clients=[64], n=0, out=None, keys=np.zeros((1, 8), U32), nonces=np.zeros((1, 3), U32), signs=[1], scale=1.0)
        args.update(kw)
        with pytest.raises(fa.FaError) as e:
            fa.secagg_unmask_device(**args)
        assert e.value.code == code and word in str(e.value), str(e.value)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(fa.ERR_ARG, "scale", scale=bad)
    T = fa.SECAGG_MAX_TERMS + 1
    refused(fa.ERR_ARG, "terms", keys=np.zeros((T, 8), U32), nonces=np.zeros((T, 3), U32), signs=np.ones(T, np.intc))
    refused(fa.ERR_ARG, "sign", signs=[0])
    refused(fa.ERR_ARG, "2^36", n=16, idx0=2 ** 36 - 15, out=64)
    refused(fa.ERR_ARG, "dtype", out_dtype=7)
    refused(fa.ERR_ARG, "D must", clients=[])
    refused(fa.ERR_ARG, "null", n=4, clients=[0], out=64)
    refused(fa.ERR_ARG, "output", n=4)
    refused(fa.ERR_ALIGN, "client", n=4, clients=[66], out=64)
    refused(fa.ERR_ALIGN, "output", n=4, out=65, out_dtype=fa.F16)
    L = fa.lib()
    assert L.fa_set_secagg(None, 0, 1.0) == fa.ERR_ARG and "ctx" in fa.last_error()
    assert L.fa_set_secagg(None, 0, float("nan")) == fa.ERR_ARG and "scale" in fa.last_error()
    assert L.fa_secagg_set_terms(None, 0, 0, None, None, None) == fa.ERR_ARG and "ctx" in fa.last_error()
    assert L.fa_secagg_mask_host(None, None, 2 ** 36 - 3, 4, None) == fa.ERR_ARG and "2^36" in fa.last_error()
    assert L.fa_secagg_mask_host(None, None, 0, 4, None) == fa.ERR_ARG and "key" in fa.last_error()
