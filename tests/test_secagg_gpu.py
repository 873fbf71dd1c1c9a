"""GPU: fa_secagg_unmask_device against tests/secagg_ref.py, exact bits -- both vector forms, the element form, heads
and tails, client passes, strided grids, every out dtype.  Receipts are random uint32 words, so every bit of the sum
matters; scale = 2^-16.
"""
import numpy as np
import pytest

import secagg_ref as SA
import server_opt_ref as S

pytestmark = pytest.mark.gpu

U32 = np.uint32
SCALE = 2.0 ** -16
PAD = 32  # guard elements around every device buffer
TOP = 2 ** 36 - 8192


def device_words(torch, host, off):
    """`host` (uint32) on the device at an element offset `off` into a guarded buffer: (buffer, the view)."""
    buf = torch.full((host.size + 2 * PAD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    view = buf[PAD + off: PAD + off + host.size]
    view.copy_(torch.from_numpy(host.view(np.int32)))
    return buf, view


# D, T, n, idx0, out kind, pointer phase agrees with the index phase, the form fa.secagg_form names, max_blocks
CASES = [
    (1, 0, 1, 0, "f32", True, 0, 0),
    (3, 1, 15, 5, "f32", True, 0, 0),
    (3, 7, 17, 4, "bf16", True, 0, 0),
    (33, 7, 1023, 0, "f16", True, 0, 0),
    (33, 1, 1025, 5, "f16", True, 0, 0),
    (3, 130, 1025, TOP, "f32", True, 1, 0),
    (3, 7, 5 * 1024 + 77, 5, "f32", True, 0, 0),
    (1, 130, 5 * 1024 + 77, 0, "bf16", True, 1, 0),
    (3, 0, 5 * 1024 + 77, TOP, "bf16", True, 0, 0),
    (3, 130, 5 * 1024 + 77, 4, "f32", False, 1, 0),  # the element form throughout
    (3, 7, 5 * 1024 + 77, 4, "f32", True, 0, 1),     # one workgroup: every tile by stride
    (130, 7, 1025, 0, "f32", True, 0, 0),            # two client passes, the sums kept in the output
    (130, 7, 1025, 5, "bf16", True, 0, 0),           # ... in the context's scratch
]


@pytest.mark.parametrize("D,T,n,idx0,okind,agree,form,max_blocks", CASES)
def test_raw_entry_equals_the_reference(fa, torch_gpu, D, T, n, idx0, okind, agree, form, max_blocks):
    torch = torch_gpu
    rng = np.random.default_rng(D * 1000 + T)
    ys = [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U32) for _ in range(D)]
    keys, nonces = rng.integers(0, 2 ** 32, (T, 8), dtype=np.uint64), rng.integers(0, 2 ** 32, (T, 3), dtype=np.uint64)
    signs = np.where(rng.integers(0, 2, T) == 1, 1, -1)
    want = S.round_out(SA.decode(SA.unmask(ys, keys, nonces, signs, idx0), SCALE), okind)
    assert fa.secagg_form(n, T) == form
    off = (idx0 + (0 if agree else 1)) % 4  # a bucket at element phase idx0 % 4 reaches 16 bytes at a multiple of 4
    held = [device_words(torch, y, off) for y in ys]
    odt = {"f32": fa.F32, "bf16": fa.BF16, "f16": fa.F16}[okind]
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[okind]
    ooff = idx0 % 4  # the output reaches its store alignment where the buckets do
    with fa.Aggregator(1) as agg:
        if max_blocks:
            agg.set_tuning(max_blocks=max_blocks)
        for forced in (None, fa.SECAGG_TILE, fa.SECAGG_SPLIT) if T else (None,):
            obuf = torch.full((n + 2 * PAD,), 7.0, dtype=tdt, device="cuda:0")
            out = obuf[PAD + ooff: PAD + ooff + n]
            torch.cuda.synchronize()  # the context's stream does not wait for torch's
            fa.secagg_unmask_device([v for _, v in held], n, out, odt, keys, nonces, signs, SCALE, idx0, form=forced,
                                    ctx=agg)
            got = out.cpu().view(torch.int32 if okind == "f32" else torch.int16).numpy()
            assert got.tobytes() == want.tobytes(), (forced, D, T, n, idx0)
            guard = torch.cat([obuf[:PAD + ooff], obuf[PAD + ooff + n:]])
            assert bool((guard == 7.0).all()), "the launch wrote outside its output"
