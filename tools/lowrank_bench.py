#!/usr/bin/env python3
"""Times low-rank receipts (fa.h "Low-rank receipts") beside the kernel and the submit they stand next to.

    tools/lowrank_bench.py [--parent-lib PATH/libfa.so] [--out profiles/lowrank_bench.json] [--reps 7] [--warmup 2]

One session, one GPU; the sides of a comparison are timed alternately, one call each per repetition, and compared by
their medians with min and max kept.

Kernel, between two events on one stream: fa_lowrank_expand_device over 64 Mi fp32 laid out as 64 matrices of 1024 x
1024, f32 against f32, at r = 4, 16 and 64, beside fa_mx8_expand_device over the same n -- the existing kernel with the
same role, one read of g and one write of x; a timed window is 10 launches, reported per launch.  The fp64
multiply-adds of the padded rank are counted from the shapes.
Host-inclusive, at C2's shape (the buckets of tests/golden/layouts/resnet18_c2.json as one part, one owner):
fa_submit_lowrank from pinned memory at r = 8, table from lowrank_mats over the tensors of at least 4096 elements, host
clock until the device has the slot, beside fa_submit_pinned of the dense receipt -- with --parent-lib on a context of
the library built from the commit before low-rank receipts, else on this library's.
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from topk_bench import ROOT, DenseSide, load_pkg, summary, timed_alternately  # noqa: E402

SIDE, COUNT = 1024, 64
INNER = 10  # launches per timed window: one launch is a fraction of a millisecond


def bench_kernel(fa, torch, np, reps, warmup):
    n = SIDE * SIDE * COUNT
    mats = [(j * SIDE * SIDE, SIDE, SIDE) for j in range(COUNT)]
    g = torch.Generator(device="cuda").manual_seed(1)
    ref = torch.rand(n, device="cuda", generator=g) * 2 - 1
    out = torch.empty_like(ref)
    q = torch.randint(-127, 128, (n,), dtype=torch.int8, device="cuda", generator=g)
    e = torch.full((fa.mx8_scale_bytes(n),), 120, dtype=torch.uint8, device="cuda")
    plan = torch.from_numpy(fa.lowrank_plan(mats, n)).cuda()
    res = {"n": n, "matrices": "%d x (%d x %d)" % (COUNT, SIDE, SIDE), "plan_bytes": plan.numel(), "ranks": {}}
    for r in (4, 16, 64):
        f = 0.1 * torch.randn(fa.lowrank_len(mats, n, r), device="cuda", generator=g)
        t = timed_alternately(torch, {
            "lowrank_expand": lambda: [fa.lowrank_expand_device(plan, f, r, n, out, ref=ref) for _ in range(INNER)],
            "mx8_expand": lambda: [fa.mx8_expand_device(q, e, n, out, ref=ref) for _ in range(INNER)]}, reps, warmup)
        t = {name: summary([ms / INNER for ms in v["ms"]]) for name, v in t.items()}  # per launch
        fa.lowrank_expand_device(plan, f, r, n, out, ref=ref)
        torch.cuda.synchronize()
        P, Q = f[:SIDE * r].view(SIDE, r).double(), f[SIDE * r:2 * SIDE * r].view(SIDE, r).double()
        want = (ref[:SIDE * SIDE].view(SIDE, SIDE) + (P @ Q.T).float())
        assert torch.allclose(out[:SIDE * SIDE].view(SIDE, SIDE), want, rtol=0, atol=1e-5), "the timed kernel's result"
        ms = t["lowrank_expand"]["median_ms"]
        fmas = n * ((r + 3) // 4 * 4)
        t.update(r=r, factor_bytes=4 * f.numel(), dense_bytes_moved=8 * n, fp64_fma=fmas,
                 fp64_tflops=2 * fmas / (ms * 1e-3) / 1e12, dense_gib_per_s=8 * n / (ms * 1e-3) / 2 ** 30,
                 ratio=ms / t["mx8_expand"]["median_ms"])
        res["ranks"]["r%d" % r] = t
    return res


def bench_submit(fa, np, parent, reps, warmup):
    with open(os.path.join(ROOT, "tests", "golden", "layouts", "resnet18_c2.json")) as fh:
        shapes = [p["shape"] for b in json.load(fh)["buckets"] for p in b["params"]]
    mats, n = fa.lowrank_mats(shapes, min_elems=4096)
    r = 8
    m = fa.lowrank_len(mats, n, r)
    rng = np.random.default_rng(2)
    pins = [fa.PinnedBuffer(4 * n), fa.PinnedBuffer(4 * m)]
    x, f = pins[0].view(np.float32), pins[1].view(np.float32)
    x[:] = np.resize(rng.uniform(-1, 1, 1 << 20).astype(np.float32), n)
    f[:] = 0.1 * rng.standard_normal(m).astype(np.float32)
    dense = DenseSide(parent if parent is not None else fa.lib(), n)
    t = {"submit_pinned_dense": [], "submit_lowrank": []}
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, 1)
        agg.set_lowrank(1, mats, r)
        agg.set_mx8_reference(1, x)
        for i in range(warmup + reps):
            a = dense.round(x)
            t0 = time.perf_counter()
            agg.submit_lowrank(1, 0, f, r, pinned=True)
            agg.sync()
            b = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                t["submit_pinned_dense"].append(a)
                t["submit_lowrank"].append(b)
    dense.lib.fa_destroy(dense.ctx)
    for p in pins:
        p.close()
    res = {name: summary(v) for name, v in t.items()}
    res.update(n=n, r=r, matrices=int(mats.size), dense_bytes=4 * n, lowrank_bytes=4 * m,
               dense_side="parent" if parent is not None else "this library",
               ratio=res["submit_lowrank"]["median_ms"] / res["submit_pinned_dense"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowrank_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "lowrank_bench.py needs a GPU"
    fa = load_pkg()
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None
    res = {"kernel": bench_kernel(fa, torch, np, a.reps, a.warmup), "submit": bench_submit(fa, np, parent, a.reps, a.warmup)}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    for name, r in list(res["kernel"]["ranks"].items()) + [("submit", res["submit"])]:
        print(name, {k: (round(v["median_ms"], 4), round(v["min_ms"], 4), round(v["max_ms"], 4)) if isinstance(v, dict) else v
                     for k, v in r.items()})


if __name__ == "__main__":
    main()
