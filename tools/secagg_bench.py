#!/usr/bin/env python3
"""Times the secagg stage (fa.h "Secagg stage") on the GPU.

    tools/secagg_bench.py [--out profiles/secagg_bench.json] [--reps 11] [--warmup 2]

North-star shape, D = 32 buckets of n = 64 Mi uint32 words: device-resident rounds through one context, fa_reduce_part
on one stream between two HIP events, alternately a plain FA_FEDAVG part (the unchanged FedAvg chain: 32 x 4 bytes
read, 4 written per element) and a secagg part with T = 0, 32 and 32 + 3 * 29 terms.  A secagg round's events also
span the upload of its term table (48 bytes per term).  From the two T > 0 medians: time per term and element, and
VALU integer instructions per second (976 per term and block of 16 elements: 960 of the rounds, 16 accumulations)
against lanes x clock, the clock and CU count being what the run's device reports.

C2's shape, D = 8 buckets of 12,557,962 words, T = 8 and 64: the two vector forms forced through the diagnostic entry,
alternately, host clock around the entry -- which uploads the table, launches and waits, the same work for both
forms, so the difference is the kernels'.
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
C2_D, C2_N = 8, 12_557_962
OPS_PER_TERM_BLOCK = 976
HIP_ATTR_CLOCK_RATE = 5  # hipDeviceAttributeClockRate: the peak clock in kHz


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def terms(np, T, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2 ** 32, (T, 8), dtype=np.uint64), rng.integers(0, 2 ** 32, (T, 3), dtype=np.uint64),
            np.where(rng.integers(0, 2, T) == 1, 1, -1))


def north_star(fa, torch, np, reps, warmup):
    stream = torch.cuda.Stream()
    counts = (0, 32, 32 + 3 * 29)
    res = {"D": D, "n": N}
    with fa.Aggregator(1) as agg:
        for part, secagg in ((1, False), (2, True)):
            agg.define(part, N, fa.F32, fa.F32, D)
            if secagg:
                agg.set_secagg(2.0 ** -16, part)
            for k in range(D):
                ptr, cnt, _ = agg.slot(part, 0, k)
                fa.fill_uniform(ptr, cnt, fa.F32, 0xD9, k)  # any bits serve as masked words
                agg.submit_commit(part, k, 1.0 / D)
        torch.cuda.synchronize()

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        def unmask(T):
            tt = terms(np, T, T)

            def run():
                agg.secagg_terms(2, *tt)
                agg.reduce(2, stream=stream)
            return run

        runs = {"plain_chain": lambda: agg.reduce(1, stream=stream)}
        runs.update({"unmask_T%d" % T: unmask(T) for T in counts})
        ts = {k: [] for k in runs}
        for i in range(warmup + reps):
            for k, fn in runs.items():
                t = event_ms(fn)
                if i >= warmup:
                    ts[k].append(t)
        for k in runs:
            res[k] = spread(ts[k])
    lo, hi = counts[1], counts[2]
    per = (res["unmask_T%d" % hi]["median_ms"] - res["unmask_T%d" % lo]["median_ms"]) * 1e-3 / ((hi - lo) * N)
    khz = ctypes.c_int()
    hip = ctypes.CDLL("libamdhip64.so")  # loaded already, by torch
    assert hip.hipDeviceGetAttribute(ctypes.byref(khz), HIP_ATTR_CLOCK_RATE, 0) == 0
    clock_hz, cus = khz.value * 1e3, torch.cuda.get_device_properties(0).multi_processor_count
    rate = OPS_PER_TERM_BLOCK / 16 / per
    res.update({"T0_over_plain_chain": res["unmask_T0"]["median_ms"] / res["plain_chain"]["median_ms"],
                "seconds_per_term_element": per, "valu_int_lane_ops_per_s": rate, "device_clock_hz": clock_hz, "device_cus": cus,
                "valu_int_peak_lane_ops_per_s": cus * 4 * 16 * clock_hz, "share_of_valu_int_peak": rate / (cus * 4 * 16 * clock_hz)})
    return res


def forms(fa, torch, np, reps, warmup):
    ys = [torch.empty(C2_N, dtype=torch.int32, device="cuda") for _ in range(C2_D)]
    for k, y in enumerate(ys):
        fa.fill_uniform(y, C2_N, fa.F32, 0xC2, k)
    out = torch.empty(C2_N, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    res = {"D": C2_D, "n": C2_N, "rule": {}}
    with fa.Aggregator(1) as agg:
        for T in (8, 64):
            tt = terms(np, T, T)
            res["rule"]["T%d" % T] = fa.secagg_form(C2_N, T)
            ts = {"tile": [], "split": []}
            for i in range(warmup + reps):
                for name, form in (("tile", fa.SECAGG_TILE), ("split", fa.SECAGG_SPLIT)):
                    t0 = time.perf_counter()
                    fa.secagg_unmask_device(ys, C2_N, out, fa.F32, *tt, 2.0 ** -16, 0, form=form, ctx=agg)
                    t = (time.perf_counter() - t0) * 1e3
                    if i >= warmup:
                        ts[name].append(t)
            res["T%d" % T] = {k: spread(v) for k, v in ts.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "secagg_bench needs a GPU"
    fa = load_pkg()
    fa.lib()
    result = {"reps": args.reps, "warmup": args.warmup, "ops_per_term_block": OPS_PER_TERM_BLOCK}
    result["north_star"] = north_star(fa, torch, np, args.reps, args.warmup)
    torch.cuda.empty_cache()
    result["c2_forms"] = forms(fa, torch, np, args.reps, args.warmup)

    def brief(v):
        return {k: brief(x) for k, x in v.items() if k != "ms"} if isinstance(v, dict) else v
    print(json.dumps(brief(result)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
