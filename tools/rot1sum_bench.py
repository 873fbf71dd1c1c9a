#!/usr/bin/env python3
"""Times a rot1-sum round (fa.h "Rot1-sum stage") beside the route it replaces, on the same commit.

    tools/rot1sum_bench.py [--out profiles/rot1sum_bench.json] [--reps 7] [--warmup 2] [--clients 8,32,64] [--n 67108864]

One session, one GPU; the two sides are timed alternately, one round each per repetition, between two events on one
stream, and compared by their medians with min and max kept.  n = 64 Mi fp32 elements, f32 reference and output, D in
{8, 32, 64} owners, once with one seed for all and once with a seed per owner:
  expanded  D calls of fa_rot1_expand_device into D dense f32 slots, then fa_reduce_device over them: what fa_submit_rot1
            and the chain enqueue;
  sum       one fa_rot1_sum_device on the same bits, scales and reference.
`ratio` is sum / expanded.  The two routes weigh the reference differently (fa.h rule 7): the bench gives weights of sum
one and compares times only; the outputs are checked to agree within the roundings of the two routes.
Byte models, per round and element: expanded 12 D + D / 8 + 4, sum D / 8 + 8.  `valu_bound_ms` is the time of 51 VALU
operations per owner and 16 elements plus 240 per transform on the device's CUs x 4 SIMDs x 16 lanes at 2.4 GHz;
`bound` names the larger of it and the sum route's bytes at 4.7 TB/s.
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
    Dmax, nb = max(clients), (n + 4095) // 4096
    slots = [torch.empty_like(g) for _ in range(Dmax)]
    bits = [torch.randint(-2 ** 31, 2 ** 31, (nb * 128,), device="cuda", generator=gen, dtype=torch.int32) for _ in range(Dmax)]
    scale = [torch.rand(nb, device="cuda", generator=gen) * 2e-4 for _ in range(Dmax)]  # |d| of about 0.01
    props = torch.cuda.get_device_properties(0)
    lanes_hz = props.multi_processor_count * 64 * 2.4e9  # VALU lane operations per second at the peak engine clock
    res = {"n": n, "device": props.name, "cus": props.multi_processor_count, "clock_hz": 2.4e9, "rounds": []}
    for D in clients:
        w = np.full(D, 1.0 / D, np.float32)
        for seeds in ("one", "distinct"):
            sd = [7] * D if seeds == "one" else list(range(100, 100 + D))

            def expanded():
                for c in range(D):
                    fa.rot1_expand_device(bits[c], scale[c], sd[c], n, slots[c], ref=g)
                fa.reduce_device(slots[:D], w, n, fa.F32, out_e)

            def summed():
                fa.rot1_sum_device(bits[:D], scale[:D], sd, n, out_s, weights=w, ref=g)

            r = timed_alternately(torch, {"expanded": expanded, "sum": summed}, reps, warmup)
            err = float((out_e - out_s).abs().max())  # not the same bits (fa.h rule 8)
            assert err < 1e-4, err
            groups = 1 if seeds == "one" else D
            valu_ms = n / 16 * (51 * D + 240 * groups) / lanes_hz * 1e3
            hbm_ms = (D / 8 + 8) * n / 4.7e12 * 1e3
            r.update(D=D, seeds=seeds, groups=groups, expanded_bytes=(12 * D + 4) * n + D * n // 8, sum_bytes=8 * n + D * n // 8,
                     max_abs_diff=err, ratio=r["sum"]["median_ms"] / r["expanded"]["median_ms"], valu_bound_ms=valu_ms,
                     hbm_bound_ms=hbm_ms, bound="VALU" if valu_ms > hbm_ms else "HBM")
            r["byte_model_ratio"] = r["sum_bytes"] / r["expanded_bytes"]
            r["sum_tb_s"] = r["sum_bytes"] / r["sum"]["median_ms"] / 1e9
            r["expanded_tb_s"] = r["expanded_bytes"] / r["expanded"]["median_ms"] / 1e9
            res["rounds"].append(r)
            print("D %d seeds %s" % (D, seeds), {s: (round(r[s]["median_ms"], 3), round(r[s]["min_ms"], 3), round(r[s]["max_ms"], 3))
                                               for s in ("expanded", "sum")},
                  "ratio %.3f (bytes %.3f) TB/s %.2f vs %.2f, VALU bound %.2f ms, HBM bound %.2f ms"
                  % (r["ratio"], r["byte_model_ratio"], r["sum_tb_s"], r["expanded_tb_s"], valu_ms, hbm_ms), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rot1sum_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clients", default="8,32,64")
    ap.add_argument("--n", type=int, default=64 * 1024 * 1024)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "rot1sum_bench.py needs a GPU"
    fa = load_pkg()
    res = bench_rounds(fa, torch, np, a.n, [int(d) for d in a.clients.split(",")], a.reps, a.warmup)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
