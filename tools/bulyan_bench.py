#!/usr/bin/env python3
"""Times the Bulyan stage's centred-mean kernel against the trimmed-mean kernel of a reference build of the
library, and a whole Bulyan round against that build's Krum round.

    tools/bulyan_bench.py --parent-lib PATH/libfa.so [--out profiles/bulyan_bench.json] [--reps 10] [--warmup 3]

--parent-lib is a libfa.so built from the commit before the Bulyan stage.  Its fa_trimmed_device over the same
theta device buffers with trim f is the yardstick of fa_centered_device with keep = theta - 2f: the same loads,
the same sort, the same window length; what the centred kernel adds is the slide of at most 2f steps and the
access to s[j + keep].  The two are timed alternately, one call each per repetition, with HIP events on one
stream, and compared by their medians; the spread (min, max) is kept.  Shapes: C2 (theta = 8), C3 (theta = 32, f32
and bf16), C4 (theta = 64) and theta = 128 (the wide form), the sizes of tools/trimmed_bench.py.

The second part times whole device-resident rounds on the north-star shape (D = 32 x 256 MiB fp32), again
alternately, host clock around fa_reduce_part and the wait for it, both driven through the C ABI alone: the
parent's Krum round (f = 7, m = D - f) and this build's Bulyan round (f = 7: theta = 18 picked, keep = 4).
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
# name, theta, f, n, dtype
SHAPES = [("c2", 8, 1, 12_557_962, "f32"), ("c3", 32, 7, 42_737_546, "f32"), ("c3_bf16", 32, 7, 42_737_546, "bf16"),
          ("c4", 64, 15, 139_611_210, "f32"), ("d128", 128, 31, 33_554_432, "f32")]
ROUND = ("north_star", 32, 7, 64 * 1024 * 1024)
P, I, S, F, U64, U32 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_uint64,
                        ctypes.c_uint32)
F32, BF16, TRIMMED, FEDAVG = 0, 1, 2, 0


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def bind(L):
    sig = {"fa_create": [ctypes.POINTER(P), I, I], "fa_destroy": [P], "fa_bucket_define": [P, I, S, I, I, I, I],
           "fa_set_krum": [P, I, I, I], "fa_bucket_slot": [P, I, I, I, ctypes.POINTER(P), ctypes.POINTER(S),
                                                           ctypes.POINTER(S)],
           "fa_fill_uniform": [P, S, I, U64, U32, U64, P], "fa_submit_commit": [P, I, I, F],
           "fa_reduce_part": [P, I, P, P], "fa_sync": [P], "fa_trimmed_device": [P, I, P, I, S, I, P, I, I, P]}
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.restype = None if name == "fa_destroy" else I
        fn.argtypes = args
    if hasattr(L, "fa_set_bulyan"):
        L.fa_set_bulyan.restype, L.fa_set_bulyan.argtypes = I, [P, I, I]
    return L


class RawRound:
    """One device-resident part of D uniform clients on a context of library L, driven through the C ABI."""

    def __init__(self, L, D, n, mode, stage):
        self.L, self.ctx = L, P()
        assert L.fa_create(ctypes.byref(self.ctx), 1, 0) == 0
        assert L.fa_bucket_define(self.ctx, 1, n, F32, F32, D, mode) == 0
        assert stage(L, self.ctx) == 0
        for k in range(D):
            ptr, cnt, off = P(), S(), S()
            assert L.fa_bucket_slot(self.ctx, 1, 0, k, ctypes.byref(ptr), ctypes.byref(cnt), ctypes.byref(off)) == 0
            assert L.fa_fill_uniform(ptr, cnt.value, F32, 0xB01A, k, 0, None) == 0
            assert L.fa_submit_commit(self.ctx, 1, k, 1.0 / D) == 0
        assert L.fa_sync(self.ctx) == 0

    def round_ms(self):
        t0 = time.perf_counter()
        assert self.L.fa_reduce_part(self.ctx, 1, None, None) == 0
        assert self.L.fa_sync(self.ctx) == 0
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.L.fa_destroy(self.ctx)


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def bench_kernel(fa, parent, torch, theta, f, n, kind, reps, warmup):
    tdt, fdt = (torch.bfloat16, fa.BF16) if kind == "bf16" else (torch.float32, fa.F32)
    clients = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(theta)]
    for k, c in enumerate(clients):
        fa.fill_uniform(c, n, fdt, 0xB01A, k)
    out = torch.empty(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    arr = (P * theta)(*[c.data_ptr() for c in clients])
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    keep = theta - 2 * f

    def trimmed():
        rc = parent.fa_trimmed_device(None, 0, arr, theta, n, fdt, out.data_ptr(), fdt, f, h)
        assert rc == 0, rc

    def centered():
        fa.centered_device(clients, n, fdt, out, fdt, keep=keep, stream=h)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    t_trim, t_cen = [], []
    for i in range(warmup + reps):
        a, b = event_ms(trimmed), event_ms(centered)
        if i >= warmup:
            t_trim.append(a)
            t_cen.append(b)
    item = 2 if kind == "bf16" else 4
    res = {"theta": theta, "f": f, "keep": keep, "n": n, "dtype": kind, "bytes": (theta + 1) * n * item,
           "parent_trimmed": spread(t_trim), "centered": spread(t_cen)}
    res["centered_over_trimmed"] = res["centered"]["median_ms"] / res["parent_trimmed"]["median_ms"]
    res["centered_GBps"] = res["bytes"] / res["centered"]["median_ms"] / 1e6
    del clients, out
    torch.cuda.empty_cache()
    return res


def bench_round(new, parent, D, f, n, reps, warmup):
    krum = RawRound(parent, D, n, FEDAVG, lambda L, ctx: L.fa_set_krum(ctx, 1, f, -1))
    bulyan = RawRound(new, D, n, TRIMMED, lambda L, ctx: L.fa_set_bulyan(ctx, 1, f))
    t_krum, t_bul = [], []
    for i in range(warmup + reps):
        a, b = krum.round_ms(), bulyan.round_ms()
        if i >= warmup:
            t_krum.append(a)
            t_bul.append(b)
    krum.close()
    bulyan.close()
    res = {"D": D, "f": f, "n": n, "krum_m": D - f, "bulyan_theta": D - 2 * f, "bulyan_keep": max(1, D - 4 * f),
           "parent_krum_round": spread(t_krum), "bulyan_round": spread(t_bul)}
    res["bulyan_over_krum"] = res["bulyan_round"]["median_ms"] / res["parent_krum_round"]["median_ms"]
    return res


def brief(d):
    return {k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "ms"}) for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    fa = load_pkg()
    new = bind(fa.lib())
    parent = bind(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    assert not hasattr(parent, "fa_set_bulyan"), "--parent-lib already has the Bulyan stage"
    result = {"reps": args.reps, "warmup": args.warmup}
    for name, theta, f, n, kind in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        result[name] = bench_kernel(fa, parent, torch, theta, f, n, kind, args.reps, args.warmup)
        print(json.dumps({name: brief(result[name])}), flush=True)
    name, D, f, n = ROUND
    if not args.only or name in args.only.split(","):
        torch.cuda.empty_cache()
        result[name] = bench_round(new, parent, D, f, n, args.reps, args.warmup)
        print(json.dumps({name: brief(result[name])}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(result, fp, indent=1)


if __name__ == "__main__":
    main()
