#!/usr/bin/env python3
"""Times the Krum stage's distance pass against the FedAvg chain of a reference build of the library, and a Krum
round against a plain one, on the north-star shape (D = 32 clients x 256 MiB fp32) and on C2's (D = 8 x 12.6 M
fp32).

    tools/krum_bench.py --parent-lib PATH/libfa.so [--out profiles/krum_bench.json] [--reps 15] [--warmup 3]

--parent-lib is a libfa.so built from the commit before the Krum stage: its fa_reduce_device over the same device
buffers is the yardstick (the distance pass reads what the chain reads and writes nothing, but does D (D - 1) / 2
subtract / convert / fp64-FMA triples per element where the chain does D FMAs).  The two are timed alternately,
one call each per repetition, with HIP events on one stream, and compared by their medians.  The distance pass
is timed as the library runs it: fa_pairdist_device on a context (the pair kernel, the kernel that adds the
partials, the read-back of the D x D matrix).

The second part times whole device-resident rounds through a context, again alternately: fa_reduce_part of a
plain part and of a Krum part (f = (D - 3) / 2, m = D - f; uniform clients, so D - m of them are left out), host
clock around the call and the wait for it.  The Krum round is the distance pass, the host's wait for its
matrix, the selection and the chain over m buffers.
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
FP32_VECTOR_PEAK = 157.3e12 / 2  # lane operations per second: the spec's FP32 vector FLOP/s, an FMA being two


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def bench_shape(fa, parent, torch, np, D, n, reps, warmup):
    P = ctypes.c_void_p
    clients = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(D)]
    for k, c in enumerate(clients):
        fa.fill_uniform(c, n, fa.F32, 0xC2A5, k)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    arr = (P * D)(*[c.data_ptr() for c in clients])
    w = np.full(D, 1.0 / D, np.float32)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    res = {"D": D, "n": n}

    with fa.Aggregator(1) as agg:
        def chain():
            rc = parent.fa_reduce_device(None, 0, arr, w.ctypes.data, D, n, fa.F32, out.data_ptr(), fa.F32, fa.FEDAVG,
                                         None, h)
            assert rc == 0, rc

        def dist():
            return fa.pairdist_device(clients, n, fa.F32, stream=h, ctx=agg)

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        t_chain, t_dist = [], []
        for i in range(warmup + reps):
            c, q = event_ms(chain), event_ms(dist)
            if i >= warmup:
                t_chain.append(c)
                t_dist.append(q)
        Q = dist()
        mc, md = statistics.median(t_chain), statistics.median(t_dist)
        triples = D * (D - 1) // 2 * n  # one fp32 subtract, one conversion, one fp64 FMA each
        res.update({"parent_chain_ms": t_chain, "dist_pass_ms": t_dist, "parent_chain_median_ms": mc,
                    "dist_pass_median_ms": md, "dist_over_chain": md / mc, "dist_bytes": D * 4 * n,
                    "dist_GBps": D * 4 * n / md / 1e6, "pair_elements": triples,
                    "lane_ops_per_s": 3 * triples / (md * 1e-3),
                    "lane_ops_over_fp32_vector_peak": 3 * triples / (md * 1e-3) / FP32_VECTOR_PEAK,
                    "q01": float(Q[0, 1]), "q01_expected_about": 2 * n / 3.0})
    del clients, out
    torch.cuda.empty_cache()

    # whole device-resident rounds: a plain part and a Krum one, alternately
    f = (D - 3) // 2
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_krum(f, None, 2)
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

        t_plain, t_krum = [], []
        for i in range(warmup + reps):
            a, b = round_ms(1), round_ms(2)
            if i >= warmup:
                t_plain.append(a)
                t_krum.append(b)
        _, _, sel = agg.krum_round(2)
        res.update({"krum_f": f, "krum_m": D - f, "selected": int(sel.sum()), "plain_round_ms": t_plain,
                    "krum_round_ms": t_krum, "plain_round_median_ms": statistics.median(t_plain),
                    "krum_round_median_ms": statistics.median(t_krum),
                    "krum_over_plain": statistics.median(t_krum) / statistics.median(t_plain)})
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
    parent.fa_reduce_device.restype = I
    parent.fa_reduce_device.argtypes = [P, I, P, P, I, S, I, P, I, I, P, P]
    assert not hasattr(parent, "fa_set_krum"), "--parent-lib already has the Krum stage"
    result = {"reps": args.reps, "warmup": args.warmup, "fp32_vector_peak_lane_ops_per_s": FP32_VECTOR_PEAK}
    for name, D, n in SHAPES:
        result[name] = bench_shape(fa, parent, torch, np, D, n, args.reps, args.warmup)
        print(json.dumps({name: {k: v for k, v in result[name].items() if not isinstance(v, list)}}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
