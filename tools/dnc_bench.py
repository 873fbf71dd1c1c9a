#!/usr/bin/env python3
"""Times the Gram pass against the Krum distance pass of a reference build of the library, and a DnC round against
a plain one, on the north-star shape (D = 32 clients x 256 MiB fp32) and on C2's (D = 8 x 12.6 M fp32).

    tools/dnc_bench.py --parent-lib PATH/libfa.so [--out profiles/dnc_bench.json] [--reps 15] [--warmup 3]

--parent-lib is a libfa.so built from the commit before the Gram pass: its fa_pairdist_device over the same device
buffers is the yardstick, the existing kernel with the same reads and the same D^2 shape (one fp32 subtract, one
conversion and one fp64 FMA per pair-element on the vector unit, where the Gram pass converts each element once and
leaves the D^2 part to the fp64 MFMA).  The two are timed alternately, one call each per repetition, with HIP events
on one stream, and compared by their medians.  Both are timed as the library runs them: the pass's kernel, the kernel
that adds the partials, the read-back of the D x D matrix; each on a context of its own library, so that neither
allocates scratch inside the timed call.

The second part times whole device-resident rounds through a context, again alternately: fa_reduce_part of a plain
part and of a DnC part (drop = (D - 1) / 2, 32 iterations; uniform clients), host clock around the call and the wait
for it.  The DnC round is the Gram pass, the host's wait for its matrix, the selection and the chain over D - drop
buffers.
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
SHAPES = [("north_star", 32, 64 * 1024 * 1024), ("c2", 8, 12_557_962)]
FP64_MATRIX_PEAK = 78.6e12 / 2  # multiply-adds per second: the spec's FP64 matrix FLOP/s, an FMA being two


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def med(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "ms": xs}


def bench_shape(fa, parent, torch, np, D, n, reps, warmup):
    P = ctypes.c_void_p
    clients = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(D)]
    for k, c in enumerate(clients):
        fa.fill_uniform(c, n, fa.F32, 0xC2A5, k)
    torch.cuda.synchronize()
    arr = (P * D)(*[c.data_ptr() for c in clients])
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    res = {"D": D, "n": n}
    pctx = P()
    assert parent.fa_create(ctypes.byref(pctx), 1, 0) == 0
    Q = np.empty((D, D), np.float64)
    try:
        with fa.Aggregator(1) as agg:
            def dist():
                rc = parent.fa_pairdist_device(pctx, 0, arr, D, n, fa.F32, Q.ctypes.data, h)
                assert rc == 0, rc

            def gram():
                return fa.gram_device(clients, n, fa.F32, stream=h, ctx=agg)

            def event_ms(fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b)

            t_dist, t_gram = [], []
            for i in range(warmup + reps):
                q, g = event_ms(dist), event_ms(gram)
                if i >= warmup:
                    t_dist.append(q)
                    t_gram.append(g)
            G = gram()
            B = (D + 15) // 16
            macs = B * (B + 1) // 2 * 256 * n  # multiply-adds the MFMAs issue, padding and mirrored halves included
            md, mg = statistics.median(t_dist), statistics.median(t_gram)
            res.update({"parent_dist_pass": med(t_dist), "gram_pass": med(t_gram), "gram_over_dist": mg / md,
                        "bytes": D * 4 * n, "gram_GBps": D * 4 * n / mg / 1e6, "dist_GBps": D * 4 * n / md / 1e6,
                        "mfma_macs": macs, "mfma_macs_over_fp64_matrix_peak": macs / (mg * 1e-3) / FP64_MATRIX_PEAK,
                        "g00": float(G[0, 0]), "g00_expected_about": n / 3.0,
                        "q01_from_gram": float(G[0, 0] + G[1, 1] - 2 * G[0, 1]), "q01_parent": float(Q[0, 1])})
    finally:
        parent.fa_destroy(pctx)
    del clients
    torch.cuda.empty_cache()

    # whole device-resident rounds: a plain part and a DnC one, alternately
    drop = (D - 1) // 2
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_dnc(drop, 32, 2)
        for part in (1, 2):
            for k in range(D):
                ptr, cnt, _ = agg.slot(part, 0, k)
                fa.fill_uniform(ptr, cnt, fa.F32, 0xC2A5, k)
                agg.submit_commit(part, k, 1.0 / D)
        torch.cuda.synchronize()

        def round_ms(part):
            t0 = time.perf_counter()
            agg.reduce(part)
            agg.sync()
            return (time.perf_counter() - t0) * 1e3

        t_plain, t_dnc = [], []
        for i in range(warmup + reps):
            a, b = round_ms(1), round_ms(2)
            if i >= warmup:
                t_plain.append(a)
                t_dnc.append(b)
        _, _, sel = agg.dnc_round(2)
        res.update({"dnc_drop": drop, "dnc_iters": 32, "selected": int(sel.sum()), "plain_round": med(t_plain),
                    "dnc_round": med(t_dnc), "dnc_over_plain": statistics.median(t_dnc) / statistics.median(t_plain)})
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
    fa = load_pkg()
    fa.lib()
    P, I, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.fa_create.restype = I
    parent.fa_create.argtypes = [ctypes.POINTER(P), I, I]
    parent.fa_destroy.restype = None
    parent.fa_destroy.argtypes = [P]
    parent.fa_pairdist_device.restype = I
    parent.fa_pairdist_device.argtypes = [P, I, P, I, S, I, P, P]
    assert not hasattr(parent, "fa_gram_device"), "--parent-lib already has the Gram pass"
    result = {"reps": args.reps, "warmup": args.warmup, "fp64_matrix_peak_macs_per_s": FP64_MATRIX_PEAK}
    for name, D, n in SHAPES:
        result[name] = bench_shape(fa, parent, torch, np, D, n, args.reps, args.warmup)
        print(json.dumps({name: {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in result[name].items()}}),
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
