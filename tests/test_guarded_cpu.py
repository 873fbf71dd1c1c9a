"""The teeth of tests/guarded.py, without a GPU: the guard checker fails on one flipped byte and names it, and
the reference of every edge-value dataset the GPU module (tests/test_kernel_forms_gpu.py) uses holds every class
it is meant to exercise, each named rounding tie on its expected bits -- so no GPU case is vacuous."""
import numpy as np
import pytest

import guarded as G


def test_guard_checker_passes_untouched_and_names_a_flipped_byte():
    for off in (0, 4, 6, 14):
        b = G.GuardedBuf(None, 1000, off)
        assert b.ptr % 16 == off and b.damage() is None
        b.check("untouched")
        b.payload()[:] = 0  # the payload is the caller's
        b.check("payload written")
        assert b.start >= G.GUARD and b.base.shape[0] - (b.start + b.nbytes) >= G.GUARD
        for at, side, rel in ((b.start - 1, "before", -1), (b.start + b.nbytes, "after", 0),
                              (0, "before", -b.start), (b.base.shape[0] - 1, "after", b.base.shape[0] - 1 - b.start - b.nbytes),
                              (b.start + b.nbytes + 777, "after", 777)):
            keep = b.base[at]
            b.base[at] ^= 0x10
            assert b.damage() == (side, rel, rel)
            with pytest.raises(AssertionError) as e:
                b.check("flipped")
            assert "%+d .. %+d" % (rel, rel) in str(e.value) and side in str(e.value)
            b.base[at] = keep
            b.check("restored")
        # a run of damaged bytes: first and last are reported
        b.base[b.start - 40:b.start - 8] = 0
        assert b.damage() == ("before", -40, -9)


def test_guard_pattern_is_nonzero_and_position_dependent():
    p = G.pattern(0, 4096)
    assert p.min() >= 1 and np.unique(p).size > 200
    assert np.array_equal(G.pattern(1000, 1100), p[1000:1100])
    assert not np.array_equal(p[:16], p[16:32])  # a 16-byte store moved by 16 bytes does not restore it


def test_nan_aware_bits():
    for dt, one, nan_a, nan_b, inf in ((G.F32, 0x3F800000, 0x7FC00000, 0xFFC00001, 0x7F800000),
                                       (G.BF16, 0x3F80, 0x7FC0, 0xFFC1, 0x7F80), (G.F16, 0x3C00, 0x7E00, 0xFE01, 0x7C00)):
        ut = G.BITS[dt]
        top = ut(1) << (31 if dt == G.F32 else 15)
        a = np.array([one, nan_a, 0, top, inf], ut)
        G.assert_bits_nan_aware(a, a.copy(), dt)
        G.assert_bits_nan_aware(a, np.array([one, nan_b, 0, top, inf], ut), dt)  # any NaN for a NaN
        for bad in ([one, nan_a, top, top, inf],   # the sign of zero counts
                    [one, inf, 0, top, inf],       # inf is not a NaN
                    [one, nan_a, 0, top, nan_a],   # a NaN where none belongs
                    [one + 1, nan_a, 0, top, inf]):
            with pytest.raises(AssertionError):
                G.assert_bits_nan_aware(a, np.array(bad, ut), dt)


@pytest.mark.parametrize("in_dt,out_dt", G.PAIRS)
def test_table_values_are_exact_in_the_input_dtype(O, in_dt, out_dt):
    G.check_table_exact(O, in_dt, out_dt)


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("D", [3, 16, 130])
@pytest.mark.parametrize("in_dt,out_dt", G.PAIRS)
def test_every_dataset_reference_holds_every_class(O, in_dt, out_dt, D, with_init):
    """The datasets of the GPU module differ in n, D, the pair and the init; the planted rows depend on the
    pair and on D only through the clients between 1 and D-1 (+0) -- checked here at a small n with seams,
    and again by every GPU case on its own reference before it touches the GPU."""
    n = 20_011
    e = G.edge_inputs(O, n, D, in_dt, out_dt, seams=(9000, 12_345), with_init=with_init)
    assert e.idx[0] == 0 and e.idx[-1] == n - 1 and np.all(np.diff(e.idx) > 0)
    for lo, hi in ((0, 4096), (n - 4096, n), (9000 - 64, 9000 + 64), (12_345 - 64, 12_345 + 64)):
        assert np.isin(np.arange(lo, hi), e.idx).all()
    assert e.idx.size >= 2 * 4096 + 2 * 128 + 50  # plus the random share
    ref, r32 = G.reference(O, e.xs, in_dt, e.w, out_dt, init=e.init)
    c = G.classes_present(e, ref, r32)
    assert c["nan"] >= 3 and c["-0"] >= 1
    # off the planted positions the data is the generator's
    rest = np.setdiff1d(np.arange(n), e.idx)
    g0 = O.gen(e.seed, 0, n, dtype="bf16") if in_dt == G.BF16 else G.to_bits(O, O.gen(e.seed, 0, n), in_dt)
    assert np.array_equal(e.xs[0][rest], g0[rest])


def test_literal_reference_classes(O):
    """The literal form sees the last client alone: its planted column holds zeros of both signs, both
    infinities, a NaN and subnormals, and fl(fl(2x) / 1000) keeps them apart."""
    for in_dt, out_dt in G.PAIRS:
        e = G.edge_inputs(O, 8200, 3, in_dt, out_dt)
        ref = G.literal_reference(O, e.xs[-1], in_dt, out_dt)
        top = G.BITS[out_dt](1) << (31 if out_dt == G.F32 else 15)
        inf = {G.F32: 0x7F800000, G.BF16: 0x7F80, G.F16: 0x7C00}[out_dt]
        assert G.nan_mask(ref, out_dt).any() and (ref == inf).any()
        assert (ref == 0).any() and (ref == top).any()
