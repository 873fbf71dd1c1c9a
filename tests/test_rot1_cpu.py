"""CPU: fa_rot1_encode and fa_rot1_decode (fa.h "Rot1 receipts") against tests/rot1_ref.py, every bit (NaN as NaN)."""
import numpy as np
import pytest

import noise_ref
import rot1_ref as R

F32, U32 = np.float32, np.uint32
B = R.B


def deltas(n, content, seed):
    rng = np.random.default_rng(seed)
    d = (F32(0.01) * rng.standard_normal(n)).astype(F32)
    blk = slice(0, min(n, B))
    if content == "zero block":
        d[blk] = 0
    elif content == "nan block":
        d[blk.stop // 2] = np.nan
    elif content == "-0 and subnormals":
        d[blk] = (rng.integers(0, 0x00800000, blk.stop).astype(U32) | (rng.integers(0, 2, blk.stop).astype(U32) << U32(31))).view(F32)
        d[0:blk.stop:3] = -0.0
    return d


@pytest.mark.parametrize("seed", [0, 0x0123456789ABCDEF])
@pytest.mark.parametrize("content", ["gaussian", "zero block", "nan block", "-0 and subnormals"])
@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 2 * B + 5])
def test_codec_is_the_rule(fa, n, content, seed):
    d = deltas(n, content, n + 1)
    bits, scale = fa.rot1_encode(d, seed)
    want_bits, want_scale = R.encode_delta(d, seed)
    what = "n %d %s" % (n, content)
    assert np.array_equal(bits, want_bits), what
    R.assert_bits(scale, want_scale, what)
    if content == "nan block":
        assert scale.view(U32)[0] == 0x7FC00000 and not bits[:R.WORDS].any()
        assert np.isnan(fa.rot1_decode(bits, scale, seed, n)[:B]).all()
    R.assert_bits(fa.rot1_decode(bits, scale, seed, n), R.decode(bits, scale, seed, 0, n), what)
    if n > 70:  # a range that starts inside a block
        R.assert_bits(fa.rot1_decode(bits, scale, seed, n - 70, idx0=64), R.decode(bits, scale, seed, 64, n - 70), what)


def test_diagonal_known_answer(fa):
    """Seed 0, elements 0 .. 127: the words of Philox counter (0, 0, 0, "ROT1") under the zero key, from the numpy
    Philox that the known answer of fa.h pins.  A block with only bit 0 set has v_0 = 4094 and v_i = -2 elsewhere, so
    the decoder's signs under scale 1 are those of v flipped by D."""
    r = noise_ref.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert " ".join("%08x" % int(w[0]) for w in r) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    words = np.concatenate(noise_ref.philox4x32_10(0, 0, 0, R.STREAM, 0, 0))
    assert " ".join("%08x" % int(w) for w in words) == DIAG_SEED0
    s = ((words[:, None] >> np.arange(32, dtype=U32)) & U32(1)).astype(bool).reshape(-1)
    bits = np.zeros(R.WORDS, U32)
    bits[0] = 1
    d = fa.rot1_decode(bits, np.ones(1, F32), 0, 128)
    assert np.array_equal(np.abs(d), np.asarray([4094] + [2] * 127, F32))
    assert np.array_equal(np.signbit(d), s ^ (np.arange(128) > 0))


DIAG_SEED0 = "8b098400 4e2160a6 db6109ce 9e26ae06"


def test_codec_nmse(fa):
    """8 blocks of N(0, 0.01^2): the reference rule gives NMSE 0.3649 against 1 - 2/pi = 0.3634; a scale wrong by a
    factor of 2 gives about 1.0 or 0.52.  It catches a wrong constant, not a rounding."""
    x = (0.01 * np.random.default_rng(0).standard_normal(8 * B)).astype(F32)
    bits, scale = fa.rot1_encode(x, 7)
    err = fa.rot1_decode(bits, scale, 7, x.size).astype(np.float64) - x
    nmse = float((err ** 2).sum() / (x.astype(np.float64) ** 2).sum())
    print("nmse", nmse)
    assert 0.33 <= nmse <= 0.40
