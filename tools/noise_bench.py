#!/usr/bin/env python3
"""Times the noise stage against the FedAvg chain of a reference build of the library, and a noisy round against
a plain one, on the north-star shape (D = 32 clients x 256 MiB fp32; the stage runs over 64 Mi fp32 in place).

    tools/noise_bench.py --parent-lib PATH/libfa.so [--out profiles/noise_bench.json] [--reps 15] [--warmup 3]

--parent-lib is a libfa.so built from the commit before the noise stage: its fa_reduce_device over the 32 device
buffers is the yardstick (the chain reads 32 x 4 bytes and writes 4 per element with 32 FMAs; the stage reads 4
and writes 4 with one Philox4x32-10 call per four elements and a logarithm, a square root, a sine and a cosine per
two).  The chain, the aligned stage (idx0 = 0) and the straddling stage (idx0 = 1: every lane's four elements
lie in two Philox groups) are timed alternately, one call each per repetition, with HIP events on one stream,
and compared by their medians.  The 16-bit forms (fp32 in, bf16 / fp16 out) are timed once each the same way.

The second part times whole device-resident rounds through a context, again alternately: fa_reduce_part of a
plain part and of a part with the stage, host clock around the call and the wait for it.
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
D, N = 32, 64 * 1024 * 1024
FP32_VECTOR_PEAK = 157.3e12 / 2  # lane operations per second: the spec's FP32 vector FLOP/s, an FMA being two
SEED = 0x0123456789ABCDEF


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def bench(fa, parent, torch, np, reps, warmup):
    P = ctypes.c_void_p
    clients = [torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(D)]
    for k, c in enumerate(clients):
        fa.fill_uniform(c, N, fa.F32, 0xD9, k)
    out = torch.empty(N, dtype=torch.float32, device="cuda")
    half = torch.empty(N, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    arr = (P * D)(*[c.data_ptr() for c in clients])
    w = np.full(D, 1.0 / D, np.float32)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    res = {"D": D, "n": N}

    with fa.Aggregator(1) as agg:
        def chain():
            rc = parent.fa_reduce_device(None, 0, arr, w.ctypes.data, D, N, fa.F32, out.data_ptr(), fa.F32, fa.FEDAVG,
                                         None, h)
            assert rc == 0, rc

        def stage(idx0, dst=None, dt=None):
            # in place on `out`: stddev 2^-20 keeps the values bounded over the repetitions
            return lambda: fa.noise_device(out, N, out if dst is None else dst, fa.F32 if dt is None else dt, 2.0 ** -20,
                                           SEED, 1, 0, idx0, stream=h, ctx=agg)

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        runs = {"parent_chain": chain, "noise_aligned": stage(0), "noise_straddling": stage(1),
                "noise_bf16_out": stage(0, half, fa.BF16), "noise_f16_out": stage(0, half, fa.F16)}
        ts = {k: [] for k in runs}
        for i in range(warmup + reps):
            for k, fn in runs.items():
                t = event_ms(fn)
                if i >= warmup:
                    ts[k].append(t)
        for k in runs:
            res[k] = spread(ts[k])
        mc = res["parent_chain"]["median_ms"]
        for k in ("noise_aligned", "noise_straddling"):
            m = res[k]["median_ms"]
            res[k].update({"over_parent_chain": m / mc, "GBps": 8 * N / m / 1e6, "normals_per_s": N / (m * 1e-3),
                           "normals_per_s_over_fp32_vector_peak": N / (m * 1e-3) / FP32_VECTOR_PEAK})
        res["parent_chain"]["GBps"] = (D + 1) * 4 * N / mc / 1e6
        for k in ("noise_bf16_out", "noise_f16_out"):
            res[k]["GBps"] = 6 * N / res[k]["median_ms"] / 1e6
    del clients, out, half
    torch.cuda.empty_cache()

    # whole device-resident rounds: a plain part and a noisy one, alternately
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        agg.define(2, N, fa.F32, fa.F32, D)
        agg.set_noise(2.0 ** -20, SEED, 2)
        for part in (1, 2):
            for k in range(D):
                ptr, cnt, _ = agg.slot(part, 0, k)
                fa.fill_uniform(ptr, cnt, fa.F32, 0xD9, k)
                agg.submit_commit(part, k, 1.0 / D)
        torch.cuda.synchronize()

        def round_ms(part):
            t0 = time.perf_counter()
            agg.reduce(part)
            agg.sync()
            return (time.perf_counter() - t0) * 1e3

        t_plain, t_noisy = [], []
        for i in range(warmup + reps):
            a, b = round_ms(1), round_ms(2)
            if i >= warmup:
                t_plain.append(a)
                t_noisy.append(b)
        res["plain_round"] = spread(t_plain)
        res["noisy_round"] = spread(t_noisy)
        res["noisy_over_plain"] = res["noisy_round"]["median_ms"] / res["plain_round"]["median_ms"]
        res["noise_rounds_used"] = agg.noise_round(2)
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
    assert not hasattr(parent, "fa_set_noise"), "--parent-lib already has the noise stage"
    result = {"reps": args.reps, "warmup": args.warmup, "fp32_vector_peak_lane_ops_per_s": FP32_VECTOR_PEAK}
    result["north_star"] = bench(fa, parent, torch, np, args.reps, args.warmup)

    def brief(v):
        return {k: x for k, x in v.items() if k != "ms"} if isinstance(v, dict) else v
    print(json.dumps({k: brief(v) for k, v in result["north_star"].items()}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
