#!/usr/bin/env python3
"""Times MX8 receipts (fa.h "MX8 receipts"): the host-inclusive round from compressed receipts against the fp32
round it replaces, the expansion kernel against the copy it follows, and the plain path against the parent's.

    tools/mx8_bench.py --parent-lib PATH/libfa.so [--out profiles/mx8_bench.json] [--reps 7] [--warmup 2]

--parent-lib is a libfa.so built from the commit before MX8 receipts; it runs on a context of its own.  One
session, one GPU; the sides of a comparison are timed alternately, one round each per repetition, and compared by
their medians with min and max kept.

Host-inclusive round, at the north star's shape (D = 32 x 64 Mi fp32) and C2's (D = 8 x 12.6 M fp32): D pinned
receipts submitted, then fa_finalize_gather into pinned memory, host clock around the whole.
  (i)   the parent's fa_submit_pinned round in fp32;
  (ii)  this library's fa_submit_mx8 round (FA_HOST_PINNED) against the part's last output;
  (iii) this library's fa_submit_pinned round in fp32 -- the unchanged path.
The receipts are four pinned buffers per kind, taken in turn (a round's PCIe bytes do not depend on their values);
(ii) / (i) is printed beside the byte ratio (33 D / 32 + 4) / (4 D + 4).

The kernel alone, at n = 64 Mi, f32 slot against an f32 reference: fa_mx8_expand_device between two events, and the
H2D copy of the n + n / 32 compressed bytes it follows, from pinned memory, the same way.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "multihop-federeated-split-learning_amd")
MI = 1024 * 1024
SHAPES = [("north_star", 32, 64 * MI), ("c2", 8, 12_557_962)]
KERNEL_N = 64 * MI
NBUF = 4
P, I, S, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
FA_F32, FA_FEDAVG, FA_HOST_PINNED = 0, 0, 1


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def declare(lib):
    for name, res, args in (("fa_create", I, [ctypes.POINTER(P), I, I]), ("fa_destroy", None, [P]),
                            ("fa_bucket_define", I, [P, I, S, I, I, I, I]), ("fa_submit_pinned", I, [P, I, I, P, F]),
                            ("fa_finalize_gather", I, [P, I, I, P, P, I]), ("fa_last_error", ctypes.c_char_p, [])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Side:
    """One library's context with one fp32 part of D x n, driven through the C ABI alone."""

    def __init__(self, lib, D, n):
        self.lib, self.D, self.n = lib, D, n
        self.ctx = P()
        self.ok(lib.fa_create(ctypes.byref(self.ctx), 1, 0))
        self.ok(lib.fa_bucket_define(self.ctx, 1, n, FA_F32, FA_F32, D, FA_FEDAVG))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.fa_last_error().decode())

    def finalize(self, dst):
        ptrs, sizes = (P * 1)(dst.ctypes.data), (S * 1)(dst.nbytes)
        self.ok(self.lib.fa_finalize_gather(self.ctx, 1, 1, ptrs, sizes, FA_HOST_PINNED))

    def full_round(self, bufs, dst):
        t0 = time.perf_counter()
        for k in range(self.D):
            self.ok(self.lib.fa_submit_pinned(self.ctx, 1, k, bufs[k % len(bufs)].ctypes.data, 1.0 / self.D))
        self.finalize(dst)
        return (time.perf_counter() - t0) * 1e3

    def mx8_round(self, qs, es, dst):
        t0 = time.perf_counter()
        for k in range(self.D):
            self.ok(self.lib.fa_submit_mx8(self.ctx, 1, k, qs[k % len(qs)].ctypes.data, es[k % len(es)].ctypes.data,
                                           1.0 / self.D, FA_HOST_PINNED))
        self.finalize(dst)
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.lib.fa_destroy(self.ctx)


def bench_rounds(fa, parent, np, D, n, reps, warmup):
    rng = np.random.default_rng(D)
    tile = rng.uniform(-1, 1, 1 << 20).astype(np.float32)
    pins, full, qs, es = [], [], [], []
    for b in range(NBUF):
        pf, pq, pe = fa.PinnedBuffer(4 * n), fa.PinnedBuffer(n), fa.PinnedBuffer(fa.mx8_scale_bytes(n))
        pins += [pf, pq, pe]
        x = pf.view(np.float32)
        x[:] = np.resize(np.roll(tile, b * 4099), n)
        q, e = pq.view(np.int8), pe.view(np.uint8)
        q[:] = np.resize(rng.integers(-127, 128, 1 << 20).astype(np.int8), n)
        e[:] = np.resize(rng.integers(120, 128, 1 << 16).astype(np.uint8), e.size)
        full.append(x)
        qs.append(q)
        es.append(e)
    pdst = fa.PinnedBuffer(4 * n)
    pins.append(pdst)
    dst = pdst.view(np.float32)
    L = fa.lib()
    old, new_full, new_mx8 = Side(parent, D, n), Side(L, D, n), Side(L, D, n)
    new_mx8.ok(L.fa_set_mx8(new_mx8.ctx, 1, 1))
    new_mx8.full_round(full, dst)  # the round that leaves the reference
    t = {"parent_fp32": [], "mx8": [], "fp32": []}
    for i in range(warmup + reps):
        a, b, c = old.full_round(full, dst), new_mx8.mx8_round(qs, es, dst), new_full.full_round(full, dst)
        if i >= warmup:
            t["parent_fp32"].append(a)
            t["mx8"].append(b)
            t["fp32"].append(c)
    assert np.isfinite(dst[:4096]).all()
    for s in (old, new_full, new_mx8):
        s.close()
    for p in pins:
        p.close()
    m = {k: statistics.median(v) for k, v in t.items()}
    spread = lambda v: max(v) - min(v)  # noqa: E731
    full_bytes, mx8_bytes = D * 4 * n + 4 * n, D * (n + fa.mx8_scale_bytes(n)) + 4 * n
    return {"D": D, "n": n, "parent_fp32_round": summary(t["parent_fp32"]), "mx8_round": summary(t["mx8"]),
            "fp32_round": summary(t["fp32"]), "mx8_over_parent_fp32": m["mx8"] / m["parent_fp32"],
            "byte_ratio": mx8_bytes / full_bytes, "fp32_over_parent_fp32": m["fp32"] / m["parent_fp32"],
            "mx8_below_parent_by_more_than_both_spreads":
                m["parent_fp32"] - m["mx8"] > spread(t["parent_fp32"]) + spread(t["mx8"]),
            "fp32_within_spreads_of_parent":
                abs(m["fp32"] - m["parent_fp32"]) <= spread(t["parent_fp32"]) + spread(t["fp32"]),
            "parent_fp32_input_GiBps": D * 4 * n / m["parent_fp32"] / 1e-3 / 2 ** 30,
            "mx8_input_GiBps": D * (n + fa.mx8_scale_bytes(n)) / m["mx8"] / 1e-3 / 2 ** 30}


def bench_kernel(fa, torch, np, n, reps, warmup):
    nb = fa.mx8_scale_bytes(n)
    q = torch.randint(-127, 128, (n,), dtype=torch.int8, device="cuda")
    e = torch.randint(120, 128, (nb,), dtype=torch.uint8, device="cuda")
    g = torch.rand(n, dtype=torch.float32, device="cuda")
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    host = torch.empty(n + nb, dtype=torch.uint8).pin_memory()
    dev = torch.empty(n + nb, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def kernel():
        fa.mx8_expand_device(q, e, n, x, fa.F32, ref=g, ref_dtype=fa.F32, stream=stream.cuda_stream)

    def copy():
        with torch.cuda.stream(stream):
            dev.copy_(host, non_blocking=True)

    tk, tc = [], []
    for i in range(warmup + reps):
        k, c = event_ms(kernel), event_ms(copy)
        if i >= warmup:
            tk.append(k)
            tc.append(c)
    moved = n + nb + 4 * n + 4 * n
    mk, mc = statistics.median(tk), statistics.median(tc)
    return {"n": n, "kernel": summary(tk), "h2d_of_compressed_bytes": summary(tc), "kernel_bytes": moved,
            "kernel_GBps": moved / mk / 1e6, "h2d_GiBps": (n + nb) / mc / 1e-3 / 2 ** 30, "kernel_over_h2d": mk / mc,
            "kernel_below_h2d": max(tk) < min(tc)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("mx8_bench: no GPU (nothing is measured without one)")
    fa = load_pkg()
    fa.lib()
    parent = declare(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    assert not hasattr(parent, "fa_submit_mx8"), "--parent-lib already has MX8 receipts"
    result = {"reps": args.reps, "warmup": args.warmup}
    result["kernel"] = bench_kernel(fa, torch, np, KERNEL_N, 3 * args.reps, args.warmup)
    print(json.dumps({"kernel": {k: v for k, v in result["kernel"].items() if not isinstance(v, dict)}}), flush=True)
    for name, D, n in SHAPES:
        result[name] = bench_rounds(fa, parent, np, D, n, args.reps, args.warmup)
        print(json.dumps({name: {k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms"})
                                 for k, v in result[name].items()}}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
