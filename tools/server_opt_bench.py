#!/usr/bin/env python3
"""Times the server-optimizer stage (fa_server_opt_device) alone and behind the FedAvg chain, against the chain
alone on the same device slots.  HIP events around `steps` back-to-back launches after `warmup`, per shape.

    tools/server_opt_bench.py [--out profiles/server_opt_bench.json] [--steps 10] [--warmup 3]

Shapes: C2 (D = 8, 12 557 962 f32), C3 (D = 32, 42 737 546 f32) and C3 in bf16.  Per rule:
  stage_ms        the stage alone, as the library runs it: in place on the fp32 aggregate for an f32 output,
                  from an fp32 aggregate buffer into a bf16 output otherwise
  chain_stage_ms  the chain into the fp32 aggregate, then the stage (one round of a part with a stage)
  chain_ms        the chain alone into the out dtype (one round of a plain part), the baseline
The stage's achieved rate comes from its algorithmic bytes per element: it reads the aggregate and the state
and writes the state and the output -- 16 + 16 B for an f32 output (12 + 12 for momentum, which has no v),
16 + 14 B for a 16-bit one (12 + 10 for momentum).  `of_spec` sets it beside 8 TB/s, the figure the sync legs'
0.71-0.73 is quoted against; the copy the microarchitecture guide measured is 6.29 TB/s.  C2's stage touches
4 x 50 MB, which fits the 256 MiB MALL: its stage-alone figure is a cache figure, chain_stage_ms is not.
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "multihop-federeated-split-learning_amd")

SHAPES = [("c2", 8, 12_557_962, "f32"), ("c3", 32, 42_737_546, "f32"), ("c3_bf16", 32, 42_737_546, "bf16")]
SPEC_TBPS = 8.0
GUIDE_COPY_TBPS = 6.29
SYNC_LEGS_OF_SPEC = [0.71, 0.73]


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
    rules = [("momentum", fa.OPT_MOMENTUM), ("adagrad", fa.OPT_ADAGRAD), ("adam", fa.OPT_ADAM), ("yogi", fa.OPT_YOGI)]
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    rows = []
    for name, D, n, kind in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        tdt, fdt, so = (torch.bfloat16, fa.BF16, 2) if kind == "bf16" else (torch.float32, fa.F32, 4)
        clients = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(D)]
        for k, c in enumerate(clients):
            fa.fill_uniform(c, n, fdt, 0x5E0F, k)
        avg = torch.empty(n, dtype=torch.float32, device="cuda")
        out = avg if kind == "f32" else torch.empty(n, dtype=tdt, device="cuda")  # f32: the stage runs in place
        plain = torch.empty(n, dtype=tdt, device="cuda")
        w = [1.0 / D] * D
        s = torch.cuda.current_stream()
        row = {"shape": name, "D": D, "n": n, "dtype": kind, "steps": args.steps, "warmup": args.warmup,
               "chain_bytes": (D * so + so) * n}
        row["chain_ms"] = timed(torch, lambda: fa.reduce_device(clients, w, n, fdt, plain, fdt, fa.FEDAVG, stream=s),
                                args.steps, args.warmup)
        for label, rule in rules:
            x = torch.zeros(n, dtype=torch.float32, device="cuda")
            m = torch.zeros(n, dtype=torch.float32, device="cuda")
            v = None if rule == fa.OPT_MOMENTUM else torch.full((n,), 0.25, dtype=torch.float32, device="cuda")
            arrays = 2 if v is None else 3

            def chain():
                fa.reduce_device(clients, w, n, fdt, avg, fa.F32, fa.FEDAVG, stream=s)

            def stage():
                fa.server_opt_device(avg, x, m, v, n, out, fdt, rule=rule, stream=s, **hp)

            def both():
                chain()
                stage()

            chain()
            stage_bytes = ((arrays + 1) * 4 + arrays * 4 + so) * n
            ms = timed(torch, stage, args.steps, args.warmup)
            row[label] = {"stage_ms": ms, "stage_bytes": stage_bytes, "stage_GBps": stage_bytes / ms / 1e6,
                          "stage_of_spec": stage_bytes / ms / 1e9 / SPEC_TBPS,
                          "stage_of_guide_copy": stage_bytes / ms / 1e9 / GUIDE_COPY_TBPS}
            ms2 = timed(torch, both, args.steps, args.warmup)
            row[label].update({"chain_stage_ms": ms2, "chain_stage_vs_chain": ms2 / row["chain_ms"],
                               "stage_behind_chain_ms": ms2 - row["chain_ms"]})
            del x, m, v
        rows.append(row)
        print(json.dumps(row), flush=True)
        del clients, avg, out, plain
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"spec_TBps": SPEC_TBPS, "guide_copy_TBps": GUIDE_COPY_TBPS,
                       "sync_legs_of_spec": SYNC_LEGS_OF_SPEC, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
