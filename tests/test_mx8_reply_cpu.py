"""CPU: MX8 replies (fa.h "MX8 replies") -- the n == 0 probe of fa_mx8_encode_device and every argument error of the
raw entry, none of which touches a device; and the invariants of the restatement the GPU tests compare against
(tests/mx8_reply_ref.py): g' within encode rule 4's bound of y, a zero delta, and the byte-maximum combine of rule 6.
"""
import numpy as np
import pytest

import mx8_ref as M
import mx8_reply_ref as P

F32, F64, I8, U8, U32 = np.float32, np.float64, np.int8, np.uint8, np.uint32


def test_probe_touches_no_device(fa):
    """n == 0 with valid arguments: FA_OK on a box without a GPU -- the feature probe."""
    for dt in (fa.F32, fa.BF16, fa.F16):
        fa.mx8_encode_device(None, None, 0, None, None, dtype=dt)
        fa.mx8_encode_device(None, None, 0, None, None, out=None, dtype=dt, idx0=2 ** 64 - 1, scales_only=True)
        fa.mx8_encode_device(None, None, 0, None, None, dtype=dt, scales_given=True)


def test_argument_errors(fa):
    def refused(code, word, *a, **k):
        with pytest.raises(fa.FaError) as ei:
            fa.mx8_encode_device(*a, **k)
        assert ei.value.code == code and word in str(ei.value), (code, word, str(ei.value))

    A = 4096  # any aligned non-null address: every refusal comes before a device call
    refused(fa.ERR_ARG, "dtype", None, None, 0, None, None, dtype=7)
    refused(fa.ERR_ARG, "dtype", None, None, 0, None, None, dtype=fa.F32, sent_dtype=-1)
    refused(fa.ERR_ARG, "one dtype", None, None, 0, None, None, dtype=fa.F32, sent_dtype=fa.BF16)
    refused(fa.ERR_ARG, "one dtype", None, None, 0, None, None, dtype=fa.F16, sent_dtype=fa.BF16)
    refused(fa.ERR_ARG, "exclude", None, None, 0, None, None, scales_only=True, scales_given=True)
    with pytest.raises(fa.FaError) as ei:
        fa.check(fa.lib().fa_mx8_encode_device(None, 0, None, fa.F32, None, fa.F32, 0, 0, None, None, None, 0x4, None))
    assert ei.value.code == fa.ERR_ARG and "flags" in str(ei.value)
    refused(fa.ERR_ARG, "2^64", None, None, 2, None, None, idx0=2 ** 64 - 1)
    refused(fa.ERR_ARG, "d_new", None, A, 4, A, A)
    refused(fa.ERR_ARG, "d_sent", A, None, 4, A, A)
    refused(fa.ERR_ARG, "d_q", A, A, 4, None, A)
    refused(fa.ERR_ARG, "d_e", A, A, 4, A, None)
    refused(fa.ERR_ARG, "d_e", A, A, 4, None, None, scales_only=True)  # q may be null there, e may not
    refused(fa.ERR_ALIGN, "d_new", A + 2, A, 4, A, A)
    refused(fa.ERR_ALIGN, "d_sent", A, A + 1, 4, A, A, dtype=fa.BF16)
    refused(fa.ERR_ALIGN, "d_out", A, 2 * A, 4, A, A, out=3 * A + 2)
    refused(fa.ERR_ALIGN, "d_out", A, 2 * A, 4, A, A, out=3 * A + 1, dtype=fa.F16)
    # aliasing: the output is an input exactly, or apart from it
    refused(fa.ERR_ARG, "overlaps d_new", A, 2 * A, 64, 3 * A, 4 * A, out=A + 4)
    refused(fa.ERR_ARG, "overlaps d_sent", A, 2 * A, 64, 3 * A, 4 * A, out=2 * A - 4)
    refused(fa.ERR_ARG, "overlaps d_sent", A, 2 * A, 64, 3 * A, 4 * A, out=2 * A + 126, dtype=fa.BF16)


# ------------------------------------------------------------------ the restatement's own invariants

def models(kind, n, seed, step=0.01):
    rng = np.random.default_rng(seed)
    sent = M.round_out(rng.uniform(-1, 1, n).astype(F32), kind)
    y = M.round_out((M.widen(sent, kind) + F32(step) * rng.standard_normal(n).astype(F32)).astype(F32), kind)
    return y, sent


@pytest.mark.parametrize("idx0", M.IDX0S)
def test_new_model_lies_within_the_encoders_bound_of_y(idx0):
    """f32: g' = fl(sent + d) with |delta - d| <= max(m / 127, 2^-134) per block (encode rule 4), so g' is within that
    bound of y plus the roundings of the subtract and of the add."""
    n = 4099
    y, sent = models("f32", n, idx0)
    q, e, g = P.reply(y, sent, "f32", idx0)
    delta = P.deltas(y, sent, "f32")
    lead = idx0 & 31
    bound = M.error_bound(np.concatenate([np.zeros(lead, F32), delta]))[lead:]
    d = M.decode(q, e, idx0)
    assert (np.abs(delta.astype(F64) - d.astype(F64)) <= bound).all()
    # the subtract rounds by at most half an ulp of delta, |delta| <= 2 max(|y|, |sent|); the add by half an ulp of g'
    ulp = np.spacing(np.maximum(np.abs(y), np.abs(sent))).astype(F64)
    assert (np.abs(g.astype(F64) - y.astype(F64)) <= bound + 2 * ulp).all()
    assert q.min() >= -127


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_zero_delta(kind):
    _, sent = models(kind, 257, 3)
    q, e, g = P.reply(sent, sent, kind, 33)
    assert (q == 0).all() and (e == 0).all()
    M.assert_bits(g, sent, "g' == sent")


def combined(delta, cut, idx0=0):
    """Rule 6 by hand: the ranges [0, cut) and [cut, n) each scale the blocks they see; the block they share takes the
    byte maximum."""
    q_lo, e_lo = P.encode_range(delta[:cut], idx0)
    q_hi, e_hi = P.encode_range(delta[cut:], idx0 + cut)
    e = np.concatenate([e_lo, e_hi])
    if (idx0 + cut) & 31:  # one block in both: its two partial scales meet
        e = np.concatenate([e_lo[:-1], [max(e_lo[-1], e_hi[0])], e_hi[1:]]).astype(U8)
    return e


def test_byte_maximum_of_partial_scales_is_the_block_scale_random_splits():
    rng = np.random.default_rng(0x6D78)
    for trial in range(200):
        n = int(rng.integers(2, 200))
        idx0 = int(rng.integers(0, 70))
        mag = 10.0 ** rng.uniform(-40, 38)
        with np.errstate(all="ignore"):
            delta = (rng.standard_normal(n) * mag * 10.0 ** rng.uniform(-3, 3, n)).astype(F32)
        cut = int(rng.integers(1, n))
        want = P.encode_range(delta, idx0)[1]
        assert np.array_equal(combined(delta, cut, idx0), want), (trial, n, idx0, cut)
        # and the codes under the combined scale are the whole block's codes
        assert np.array_equal(P.codes_under(delta, want, idx0), P.encode_range(delta, idx0)[0]), trial


def edge_max(E, top):
    """The largest (top) or smallest maximum whose block scale is E, as fp32: 127 * 2^(E - 133) and the value after
    127 * 2^(E - 134)."""
    if top:
        return F32(np.ldexp(127.0, E - 133)) if E < 254 else np.finfo(F32).max
    if E == 0:
        return F32(2.0 ** -149)
    return np.nextafter(F32(np.ldexp(127.0, E - 134)), F32(np.inf))


@pytest.mark.parametrize("E", [0, 1, 6, 7, 254, 255])
def test_byte_maximum_at_the_scale_edges(E):
    """The block maximum at both ends of E's interval, on either side of the cut; 255 from a NaN or an inf."""
    small = F32(2.0 ** -149)
    for top in (False, True):
        for side in (0, 1):
            for cut in (1, 13, 31):
                delta = np.full(32, small, F32)
                at = 0 if side == 0 else 31
                delta[at] = edge_max(E, top) if E < 255 else (np.nan if top else -np.inf)
                whole = P.encode_range(delta)[1]
                assert whole[0] == E, (E, top, float(delta[at]), whole)
                got = combined(delta, cut)
                assert np.array_equal(got, whole), (E, top, side, cut)
                lo, hi = P.encode_range(delta[:cut])[1][0], P.encode_range(delta[cut:], cut)[1][0]
                assert max(lo, hi) == E and min(lo, hi) <= E
