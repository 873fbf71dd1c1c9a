#!/usr/bin/env python3
"""Times rot1 receipts (fa.h "Rot1 receipts") beside the MX8 kernels they stand next to.

    tools/rot1_bench.py [--out profiles/rot1_bench.json] [--reps 7] [--warmup 2]

One session, one GPU; the sides of a comparison are timed alternately, one call each per repetition, and compared by
their medians with min and max kept.

Kernels, at n = 64 Mi fp32, between two events on one stream:
  encode   fa_rot1_encode_device, g' written into a buffer of its own, beside fa_mx8_encode_device's fused pass on the
           same new and sent;
  expand   fa_rot1_expand_device beside fa_mx8_expand_device, f32 against f32.
Host-inclusive, at C2's shape (12.6 M fp32 elements, one owner): fa_submit_rot1 from pinned memory, host clock until
the device has the slot, beside fa_submit_pinned of the dense receipt on a context of the same library.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "multihop-federeated-split-learning_amd")
MI = 1024 * 1024
KERNEL_N, C2_N = 64 * MI, 12_557_962


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def timed_alternately(torch, sides, reps, warmup):
    """sides: name -> callable that enqueues one call on the current stream; per name the event times in ms."""
    t = {name: [] for name in sides}
    for i in range(warmup + reps):
        for name, call in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if i >= warmup:
                t[name].append(a.elapsed_time(b))
    return {name: summary(v) for name, v in t.items()}


def bench_kernels(fa, torch, reps, warmup):
    n, seed = KERNEL_N, 7
    g = torch.Generator(device="cuda").manual_seed(1)
    sent = torch.rand(n, device="cuda", generator=g) * 2 - 1
    new = sent + 0.05 * torch.randn(n, device="cuda", generator=g)
    out = torch.empty_like(sent)
    q = torch.empty(n, dtype=torch.int8, device="cuda")
    e = torch.empty(fa.mx8_scale_bytes(n), dtype=torch.uint8, device="cuda")
    nb = fa.rot1_blocks(n)
    bits = torch.empty(nb * 128, dtype=torch.int32, device="cuda")
    scale = torch.empty(nb, dtype=torch.float32, device="cuda")
    res = {"n": n}
    r = timed_alternately(torch, {
        "rot1_encode": lambda: fa.rot1_encode_device(new, sent, n, seed, bits, scale, out=out),
        "mx8_encode": lambda: fa.mx8_encode_device(new, sent, n, q, e, out=out)}, reps, warmup)
    assert torch.isfinite(scale).all() and (scale > 0).all()
    r.update(rot1_bytes_per_element=12 + 516 / 4096, mx8_bytes_per_element=13 + 1 / 32,
             ratio=r["rot1_encode"]["median_ms"] / r["mx8_encode"]["median_ms"])
    res["encode"] = r
    r = timed_alternately(torch, {
        "rot1_expand": lambda: fa.rot1_expand_device(bits, scale, seed, n, out, ref=sent),
        "mx8_expand": lambda: fa.mx8_expand_device(q, e, n, out, ref=sent)}, reps, warmup)
    # out: the last side's expansion, MX8's
    nmse = float(((out - new).double() ** 2).sum() / ((new - sent).double() ** 2).sum())
    fa.rot1_expand_device(bits, scale, seed, n, out, ref=sent)
    nmse_rot1 = float(((out - new).double() ** 2).sum() / ((new - sent).double() ** 2).sum())
    r.update(rot1_bytes_per_element=8 + 516 / 4096, mx8_bytes_per_element=9 + 1 / 32, nmse_rot1=nmse_rot1, nmse_mx8=nmse,
             ratio=r["rot1_expand"]["median_ms"] / r["mx8_expand"]["median_ms"])
    for side in ("rot1", "mx8"):
        r[side + "_gbytes_per_s"] = r[side + "_bytes_per_element"] * n / r[side + "_expand"]["median_ms"] / 1e6
    res["expand"] = r
    return res


def bench_submit(fa, np, reps, warmup):
    n = C2_N
    nb = fa.rot1_blocks(n)
    rng = np.random.default_rng(2)
    pins = [fa.PinnedBuffer(4 * n), fa.PinnedBuffer(4 * 128 * nb), fa.PinnedBuffer(4 * nb)]
    x, bits, scale = pins[0].view(np.float32), pins[1].view(np.uint32), pins[2].view(np.float32)
    x[:] = np.resize(rng.uniform(-1, 1, 1 << 20).astype(np.float32), n)
    bits[:] = rng.integers(0, 1 << 32, bits.size, dtype=np.uint64).astype(np.uint32)
    scale[:] = 1e-3
    t = {"submit_pinned_dense": [], "submit_rot1": []}
    with fa.Aggregator(1) as dense, fa.Aggregator(1) as agg:
        dense.define(1, n, fa.F32, fa.F32, 1)
        agg.define(1, n, fa.F32, fa.F32, 1)
        agg.set_rot1(True, 1)
        agg.set_mx8_reference(1, x)
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            dense.submit(1, 0, x, pinned=True)
            dense.sync()
            a = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            agg.submit_rot1(1, 0, bits, scale, 7, pinned=True)
            agg.sync()
            b = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                t["submit_pinned_dense"].append(a)
                t["submit_rot1"].append(b)
    for p in pins:
        p.close()
    r = {name: summary(v) for name, v in t.items()}
    r.update(n=n, dense_bytes=4 * n, rot1_bytes=516 * nb,
             ratio=r["submit_rot1"]["median_ms"] / r["submit_pinned_dense"]["median_ms"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rot1_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "rot1_bench.py needs a GPU"
    fa = load_pkg()
    res = {"kernels": bench_kernels(fa, torch, a.reps, a.warmup), "submit": bench_submit(fa, np, a.reps, a.warmup)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for name, r in (("encode", res["kernels"]["encode"]), ("expand", res["kernels"]["expand"]), ("submit", res["submit"])):
        print(name, {k: (round(v["median_ms"], 4), round(v["min_ms"], 4), round(v["max_ms"], 4)) if isinstance(v, dict) else v
                     for k, v in r.items()})


if __name__ == "__main__":
    main()
