#!/usr/bin/env python3
"""Times an MX8-sum round (fa.h "MX8-sum stage") beside the route it replaces, on the same commit.

    tools/mx8sum_bench.py [--out profiles/mx8sum_bench.json] [--reps 7] [--warmup 2] [--clients 8,32,64] [--n 67108864]

One session, one GPU; the two sides are timed alternately, one round each per repetition, between two events on one
stream, and compared by their medians with min and max kept.  n = 64 Mi fp32 elements, f32 reference and output, D in
{8, 32, 64} owners:
  expanded  D calls of fa_mx8_expand_device into D dense f32 slots, then fa_reduce_device over them: what fa_submit_mx8
            and the chain enqueue;
  sum       one fa_mx8_sum_device on the same codes, scales and reference.
`ratio` is sum / expanded.  The two routes weigh the reference differently (fa.h rule 4): the bench gives weights of sum
one and compares times only; the outputs are checked to agree within the roundings of the expanded route.
Byte models, per round: expanded (13 + 1 / 32) D n + 4 n, sum (1 + 1 / 32) D n + 8 n.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "multihop-federeated-split-learning_amd")


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def timed_alternately(torch, sides, reps, warmup):
    """sides: name -> callable that enqueues one round on the current stream; per name the event times in ms."""
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


def bench_rounds(fa, torch, np, n, clients, reps, warmup):
    gen = torch.Generator(device="cuda").manual_seed(1)
    g = torch.rand(n, device="cuda", generator=gen) * 2 - 1
    out_e, out_s = torch.empty_like(g), torch.empty_like(g)
    Dmax, nb = max(clients), (n + 31) // 32
    slots = [torch.empty_like(g) for _ in range(Dmax)]
    q = [torch.randint(-127, 128, (n,), device="cuda", generator=gen, dtype=torch.int8) for _ in range(Dmax)]
    e = [torch.randint(110, 120, (nb,), device="cuda", generator=gen, dtype=torch.uint8) for _ in range(Dmax)]  # |d| < 2^-6
    res = {"n": n, "rounds": []}
    for D in clients:
        w = np.full(D, 1.0 / D, np.float32)

        def expanded():
            for c in range(D):
                fa.mx8_expand_device(q[c], e[c], n, slots[c], ref=g)
            fa.reduce_device(slots[:D], w, n, fa.F32, out_e)

        def summed():
            fa.mx8_sum_device(q[:D], e[:D], n, out_s, weights=w, ref=g)

        assert fa.mx8_sum_form(n, q[:D], out_s, fa.F32, g, fa.F32) == fa.MX8_SUM_VECTOR
        r = timed_alternately(torch, {"expanded": expanded, "sum": summed}, reps, warmup)
        err = float((out_e - out_s).abs().max())  # not the same bits (fa.h rule 5): D roundings of g + d_c at |g| < 1
        assert err < 1e-5, err
        r.update(D=D, expanded_bytes=(13 * D + 4) * n + D * nb, sum_bytes=(D + 8) * n + D * nb, max_abs_diff=err,
                 ratio=r["sum"]["median_ms"] / r["expanded"]["median_ms"])
        r["sum_tb_s"] = r["sum_bytes"] / r["sum"]["median_ms"] / 1e9
        r["expanded_tb_s"] = r["expanded_bytes"] / r["expanded"]["median_ms"] / 1e9
        res["rounds"].append(r)
        print("D %d" % D, {s: (round(r[s]["median_ms"], 3), round(r[s]["min_ms"], 3), round(r[s]["max_ms"], 3))
                           for s in ("expanded", "sum")},
              "ratio %.3f TB/s %.2f vs %.2f" % (r["ratio"], r["sum_tb_s"], r["expanded_tb_s"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8sum_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clients", default="8,32,64")
    ap.add_argument("--n", type=int, default=64 * 1024 * 1024)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "mx8sum_bench.py needs a GPU"
    fa = load_pkg()
    res = bench_rounds(fa, torch, np, a.n, [int(d) for d in a.clients.split(",")], a.reps, a.warmup)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
