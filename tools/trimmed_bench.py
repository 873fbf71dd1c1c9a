#!/usr/bin/env python3
"""Times the FA_TRIMMED kernel against the FedAvg chain on the same device slots (the chain moves the same
bytes, so its time is the floor).  HIP events around `steps` back-to-back launches after `warmup`, per shape.

    tools/trimmed_bench.py [--out profiles/trimmed_bench.json] [--steps 10] [--warmup 3]

Shapes: C2 (D = 8, 12 557 962 f32), C3 (D = 32, 42 737 546 f32), C3 in bf16, C4 (D = 64, 139 611 210 f32), and
D = 128 over 2^25 f32 (the wide form); every working set is far beyond the 256 MiB MALL.  Trims: 1 and the median.
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "multihop-federeated-split-learning_amd")

SHAPES = [("c2", 8, 12_557_962, "f32"), ("c3", 32, 42_737_546, "f32"), ("c3_bf16", 32, 42_737_546, "bf16"),
          ("c4", 64, 139_611_210, "f32"), ("d128", 128, 33_554_432, "f32")]


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    fa = load_pkg()
    rows = []
    for name, D, n, kind in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        tdt, fdt = (torch.bfloat16, fa.BF16) if kind == "bf16" else (torch.float32, fa.F32)
        clients = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(D)]
        for k, c in enumerate(clients):
            fa.fill_uniform(c, n, fdt, 0x7121, k)
        out = torch.empty(n, dtype=tdt, device="cuda")
        w = [1.0 / D] * D
        s = torch.cuda.current_stream()
        row = {"shape": name, "D": D, "n": n, "dtype": kind, "steps": args.steps, "warmup": args.warmup,
               "bytes": (D + 1) * n * (2 if kind == "bf16" else 4)}
        row["chain_ms"] = timed(torch, lambda: fa.reduce_device(clients, w, n, fdt, out, fdt, fa.FEDAVG, stream=s),
                                args.steps, args.warmup)
        for label, trim in (("trim1", 1), ("median", fa.TRIM_MEDIAN)):
            ms = timed(torch, lambda: fa.trimmed_device(clients, n, fdt, out, fdt, trim=trim, stream=s), args.steps,
                       args.warmup)
            row[label + "_ms"] = ms
            row[label + "_vs_chain"] = ms / row["chain_ms"]
            row[label + "_GBps"] = row["bytes"] / ms / 1e6
        rows.append(row)
        print(json.dumps(row), flush=True)
        del clients, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
