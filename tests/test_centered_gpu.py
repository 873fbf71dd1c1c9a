"""GPU: fa_centered_device (fa.h "Bulyan stage", rule 4) against tests/bulyan_ref.py, every bit.

theta covers every padded width P = 2 .. 64, both sides of each boundary and the wide form (65 .. 128); keep the
ends and the middle of 1 .. theta; n the head alone, the tail, one and several vectors; every dtype pair; three
pointer layouts (all at 16-byte phase 0: the vector form; a shared phase of one element: head + vectors + tail;
mixed phases: the element form) in guarded buffers, so a store outside the output shows.  The inputs are random
normals with the special columns of bulyan_ref.special_columns planted in the head, the body and the tail.  The
expected values of one theta are computed once per (input kind, n, keep) and shared by the out dtypes and layouts.
"""
import numpy as np
import pytest

import bulyan_ref as B
from guarded import PAIRS, GuardedBuf, assert_unchanged, snapshot

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0xCE47
THETAS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 96, 128]
NS = [1, 7, 67, 4099]
ITEM = {"f32": 4, "bf16": 2, "f16": 2}


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def keeps(theta):
    return sorted({k for k in (1, 2, theta // 2 + 1, theta - 1, theta) if 1 <= k <= theta})


def make_inputs(theta, n, kind):
    """theta buckets of `kind`: normals, with the special columns at the start, the middle and the end."""
    rng = np.random.default_rng(SEED + 1000 * theta + n)
    x = rng.normal(size=(theta, n)).astype(F32)
    cols = B.special_columns(theta)
    for base in (0, n // 2, n - len(cols)):
        for c, col in enumerate(cols):
            if 0 <= base + c < n:
                x[:, base + c] = col
    return [B.round_out(x[k], kind) for k in range(theta)]


def layouts(theta, kind):
    """Per-client 16-byte phases in elements: all 0, one shared phase, mixed."""
    per = 16 // ITEM[kind]
    return {"phase 0": [0] * theta, "shared phase 1": [1] * theta, "mixed": [k % per for k in range(theta)]}


def upload(torch, xs, kind, offsets):
    tdt = torch.int32 if kind == "f32" else torch.int16
    ndt = np.int32 if kind == "f32" else np.int16
    bufs, views, snaps = [], [], []
    for x, o in zip(xs, offsets):
        b = GuardedBuf(torch, x.size * ITEM[kind], o * ITEM[kind])
        v = b.view(tdt)
        v.copy_(torch.from_numpy(np.ascontiguousarray(x).view(ndt)))
        bufs.append(b)
        views.append(v)
        snaps.append(snapshot(v))
    return bufs, views, snaps


def read_out(torch, buf, okind, n):
    tdt = torch.int32 if okind == "f32" else torch.int16
    raw = buf.view(tdt).cpu().numpy()
    return raw.view({"f32": np.float32, "f16": np.float16, "bf16": np.uint16}[okind])[:n]


@pytest.mark.parametrize("in_kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("theta", THETAS)
def test_centered_device_matches_the_rule_in_all_bits(fa, torch_gpu, theta, in_kind):
    torch = torch_gpu
    outs = [o for i, o in PAIRS if i == in_kind]
    for n in NS:
        xs = make_inputs(theta, n, in_kind)
        wide = [B.widen(x, in_kind) for x in xs]
        refs = {keep: B.centered_f32(wide, keep)[0] for keep in keeps(theta)}
        for name, offsets in layouts(theta, in_kind).items():
            bufs, views, snaps = upload(torch, xs, in_kind, offsets)
            ptrs = [b.ptr for b in bufs]
            for okind in outs:
                # the output shares the clients' phase in bytes where they share one, else it sits at phase 0
                ophase = offsets[0] * ITEM[in_kind] if len(set(offsets)) == 1 else 0
                if ophase % ITEM[okind]:
                    ophase = 0
                for keep in keeps(theta):
                    out = GuardedBuf(torch, n * ITEM[okind], ophase)
                    fa.centered_device(ptrs, n, fa_dt(fa, in_kind), out.ptr, fa_dt(fa, okind), keep=keep)
                    torch.cuda.synchronize()
                    what = "theta %d keep %d n %d %s -> %s, %s" % (theta, keep, n, in_kind, okind, name)
                    B.assert_bits(read_out(torch, out, okind, n), B.round_out(refs[keep], okind), what)
                    out.check(what)
            for k in range(theta):
                bufs[k].check("theta %d n %d %s client %d" % (theta, n, name, k))
                assert_unchanged(views[k], snaps[k], "theta %d n %d %s client %d" % (theta, n, name, k))


@pytest.mark.parametrize("in_kind,okind", PAIRS)
def test_keep_theta_is_the_trimmed_mean_with_trim_0(fa, torch_gpu, in_kind, okind):
    torch = torch_gpu
    n = 4099
    for theta in (1, 3, 8, 17, 33, 65, 128):
        xs = make_inputs(theta, n, in_kind)
        bufs, _, _ = upload(torch, xs, in_kind, [0] * theta)
        ptrs = [b.ptr for b in bufs]
        a, b = GuardedBuf(torch, n * ITEM[okind]), GuardedBuf(torch, n * ITEM[okind])
        fa.centered_device(ptrs, n, fa_dt(fa, in_kind), a.ptr, fa_dt(fa, okind), keep=theta)
        fa.trimmed_device(ptrs, n, fa_dt(fa, in_kind), b.ptr, fa_dt(fa, okind), trim=0)
        torch.cuda.synchronize()
        got, ref = read_out(torch, a, okind, n), read_out(torch, b, okind, n)
        B.assert_bits(got, ref, "theta %d %s -> %s: keep == theta is trim 0" % (theta, in_kind, okind))
        a.check("centred")


def test_a_capped_grid_strides_over_the_bucket(fa, torch_gpu):
    """Three workgroups for 100003 elements: the grid-stride loops of the three forms."""
    torch = torch_gpu
    n = 100003
    for theta, keep, offsets in ((8, 4, None), (40, 8, None), (70, 30, None), (8, 4, "mixed")):
        xs = make_inputs(theta, n, "f32")
        offs = [k % 4 for k in range(theta)] if offsets else [0] * theta
        bufs, _, _ = upload(torch, xs, "f32", offs)
        ref = B.centered_f32(xs, keep)[0]
        with fa.Aggregator(1) as agg:
            agg.set_tuning(max_blocks=3)
            out = GuardedBuf(torch, n * 4)
            fa.centered_device([b.ptr for b in bufs], n, fa.F32, out.ptr, fa.F32, keep=keep, ctx=agg)
            torch.cuda.synchronize()
            B.assert_bits(read_out(torch, out, "f32", n), ref, "3 workgroups, theta %d" % theta)
            out.check("3 workgroups, theta %d" % theta)
