"""CPU: fa_topk_encode and fa_topk_decode (fa.h "Top-k receipts", rules 2-5 and the decoder) against tests/topk_ref.py,
every bit (NaN as NaN): random deltas, all-equal and +-0-only keys (ties cut by index alone), two values with the cut
inside a run, NaN, +-inf and subnormals, for k from 0 to beyond n."""
import numpy as np
import pytest

import topk_ref as K

NS = [1, 33, 1000]


@pytest.mark.parametrize("pattern", ["random", "equal", "pm0", "specials", "subnormal", "two"])
@pytest.mark.parametrize("n", NS)
def test_encode_and_decode_against_the_reference(fa, n, pattern):
    delta = K.deltas(pattern, n, n)
    for k in (0, 1, n // 2, n, n + 5):
        what = "%s n %d k %d" % (pattern, n, k)
        idx, val = fa.topk_encode(delta, k)
        want_idx, want_val = K.select(delta, k)
        assert idx.dtype == np.uint32 and np.array_equal(idx, want_idx), what
        K.assert_bits(val, want_val, what)
        for idx0, m in ((0, n), (n // 3, n // 2), (7, n + 9)):
            K.assert_bits(fa.topk_decode(idx, val, m, idx0), K.decode(want_idx, want_val, m, idx0), what)


def test_decode_refuses_indices_that_do_not_ascend(fa):
    for idx in ([3, 3], [5, 2], [0, 4, 4, 9]):
        with pytest.raises(fa.FaError) as ei:
            fa.topk_decode(np.asarray(idx, np.uint32), np.ones(len(idx), np.float32), 16)
        assert ei.value.code == fa.ERR_ARG and "ascending" in str(ei.value)
