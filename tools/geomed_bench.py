#!/usr/bin/env python3
"""Times the geomed stage's fused Weiszfeld pass against what one Weiszfeld iteration cost before it existed, and
a geomed round against a plain one.

    tools/geomed_bench.py --parent-lib PATH/libfa.so [--out profiles/geomed_bench.json] [--reps 15] [--warmup 3]

--parent-lib is a libfa.so built from the commit before the geomed stage.  Over the same device buffers its
(i) fa_reduce_device chain into an f32 buffer and (ii) fa_clip_sumsq_device against that buffer are the yardstick:
their sum is one iteration done with the two existing passes (the buckets read twice, v written and read back);
both run on a context of the parent's, so its measure pass keeps its scratch across calls as the fused one does.
The fused pass (fa_geomed_pass_device on a context, v not stored, as the stage calls it: the kernel, the kernel
that adds the partials, the read-back of the 2 D numbers) must take less than (i) + (ii) at D <= 32, or fusing is
pointless.  The three are timed alternately, one call each per repetition, with HIP events on one stream, and
compared by their medians; min and max are kept.

Shapes: the north star (D = 32 x 256 MiB fp32), C2's (D = 8 x 12.6 M fp32), the wide forms D = 64 and D = 128 at
8 GiB of fp32, and bf16 at D = 32 x 64 Mi elements.

The second part times whole device-resident rounds through a context at the north star, again alternately:
fa_reduce_part of a plain part and of geomed parts with T = 3 and T = 8, host clock around the call and the wait
for it.  A geomed round is T fused passes, each with a host wait and the weights rule, then the chain.
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
SHAPES = [("north_star", 32, 64 * MI, "f32"), ("c2", 8, 12_557_962, "f32"), ("wide_64", 64, 32 * MI, "f32"),
          ("wide_128", 128, 16 * MI, "f32"), ("bf16_32", 32, 64 * MI, "bf16")]
ROUND_SHAPE = (32, 64 * MI)
ROUND_T = (3, 8)


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def bench_pass(fa, parent, pctx, torch, np, D, n, kind, reps, warmup):
    P = ctypes.c_void_p
    dt, tdt, item = (fa.F32, torch.float32, 4) if kind == "f32" else (fa.BF16, torch.bfloat16, 2)
    clients = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(D)]
    for k, c in enumerate(clients):
        fa.fill_uniform(c, n, dt, 0x6E0D, k)
    v = torch.empty(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    arr = (P * D)(*[c.data_ptr() for c in clients])
    w = np.full(D, 1.0 / D, np.float32)
    q_parent = np.empty(D, np.float64)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    res = {"D": D, "n": n, "dtype": kind, "bytes": D * item * n}

    with fa.Aggregator(1) as agg:
        def chain():
            rc = parent.fa_reduce_device(pctx, 0, arr, w.ctypes.data, D, n, dt, v.data_ptr(), fa.F32, fa.FEDAVG, None, h)
            assert rc == 0, rc

        def sumsq():
            rc = parent.fa_clip_sumsq_device(pctx, 0, arr, D, n, dt, v.data_ptr(), q_parent.ctypes.data, h)
            assert rc == 0, rc

        def fused():
            return fa.geomed_pass_device(clients, w, n, dt, stream=h, ctx=agg)

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        t_chain, t_sumsq, t_fused = [], [], []
        for i in range(warmup + reps):
            c, s, f = event_ms(chain), event_ms(sumsq), event_ms(fused)
            if i >= warmup:
                t_chain.append(c)
                t_sumsq.append(s)
                t_fused.append(f)
        q, b = fused()
        mc, ms, mf = (statistics.median(t) for t in (t_chain, t_sumsq, t_fused))
        worst = float(np.max(np.abs(q - q_parent) / q_parent))  # the same v bits: two orders of the same sum
        res.update({"parent_chain": summary(t_chain), "parent_sumsq": summary(t_sumsq), "fused": summary(t_fused),
                    "two_passes_median_ms": mc + ms, "fused_over_two_passes": mf / (mc + ms),
                    "fused_over_parent_chain": mf / mc, "parent_sumsq_over_parent_chain": ms / mc,
                    "fused_GBps": D * item * n / mf / 1e6, "nonfinite": float(b.sum()),
                    "q_relative_difference_to_parent_max": worst})
    del clients, v
    torch.cuda.empty_cache()
    return res


def bench_rounds(fa, torch, D, n, reps, warmup):
    res = {"D": D, "n": n}
    with fa.Aggregator(1) as agg:
        parts = {0: 1}
        agg.define(1, n, fa.F32, fa.F32, D)
        for i, T in enumerate(ROUND_T):
            parts[T] = 2 + i
            agg.define(2 + i, n, fa.F32, fa.F32, D)
            agg.set_geomed(T, 1e-6, 2 + i)
        for part in parts.values():
            for k in range(D):
                ptr, cnt, _ = agg.slot(part, 0, k)
                fa.fill_uniform(ptr, cnt, fa.F32, 0x6E0D, k)
                agg.submit_commit(part, k, 1.0 / D)
        torch.cuda.synchronize()

        def round_ms(part):
            t0 = time.perf_counter()
            agg.reduce(part)
            agg.sync()
            return (time.perf_counter() - t0) * 1e3

        ts = {T: [] for T in parts}
        for i in range(warmup + reps):
            for T, part in parts.items():
                t = round_ms(part)
                if i >= warmup:
                    ts[T].append(t)
        plain = statistics.median(ts[0])
        res["plain_round"] = summary(ts[0])
        for T in ROUND_T:
            q, wr, inc, obj = agg.geomed_round(parts[T])
            res["geomed_T%d_round" % T] = dict(summary(ts[T]), passes=int(q.shape[0]), included=int(inc.sum()),
                                               over_plain=statistics.median(ts[T]) / plain)
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("geomed_bench: no GPU (nothing is measured without one)")
    fa = load_pkg()
    fa.lib()
    P, I, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.fa_reduce_device.restype = I
    parent.fa_reduce_device.argtypes = [P, I, P, P, I, S, I, P, I, I, P, P]
    parent.fa_clip_sumsq_device.restype = I
    parent.fa_clip_sumsq_device.argtypes = [P, I, P, I, S, I, P, P, P]
    assert not hasattr(parent, "fa_set_geomed"), "--parent-lib already has the geomed stage"
    # a context of the parent's own: its measure pass then keeps its scratch across calls, as ours does
    parent.fa_create.restype = I
    parent.fa_create.argtypes = [ctypes.POINTER(P), I, I]
    parent.fa_destroy.restype = None
    parent.fa_destroy.argtypes = [P]
    pctx = P()
    assert parent.fa_create(ctypes.byref(pctx), 1, 0) == 0
    result = {"reps": args.reps, "warmup": args.warmup}
    for name, D, n, kind in SHAPES:
        result[name] = bench_pass(fa, parent, pctx, torch, np, D, n, kind, args.reps, args.warmup)
        print(json.dumps({name: {k: v for k, v in result[name].items() if not isinstance(v, dict)}}), flush=True)
    parent.fa_destroy(pctx)
    result["rounds_north_star"] = bench_rounds(fa, torch, *ROUND_SHAPE, args.reps, args.warmup)
    print(json.dumps({"rounds_north_star": {k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms"})
                                            for k, v in result["rounds_north_star"].items()}}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
