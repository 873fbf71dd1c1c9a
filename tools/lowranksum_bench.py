#!/usr/bin/env python3
"""Times a low-rank-sum round (fa.h "Low-rank-sum stage") beside the route it replaces, on the same commit.

    tools/lowranksum_bench.py [--out profiles/lowranksum_bench.json] [--reps 7] [--warmup 2] [--clients 8,32,64]
                              [--ranks 4,16,64] [--mats 64] [--side 1024]

One session, one GPU; the two sides are timed alternately, one round each per repetition, between two events on one
stream, and compared by their medians with min and max kept.  The bucket is `mats` matrices of side x side fp32 (no rest),
f32 reference and output, every owner of the same rank r:
  expanded  D calls of fa_lowrank_expand_device into D dense f32 slots, then fa_reduce_device over them: what
            fa_submit_lowrank and the chain enqueue;
  sum       one fa_lowrank_sum_device on the same receipts and reference.
`ratio` is sum / expanded.  The two routes weigh the reference differently (fa.h rule 5): the bench gives weights of sum one
and compares times only; the outputs are checked to agree within the roundings of the expanded route.
Byte models, per element: expanded 12 D + 4, sum 8.  `sum_tflops` counts 2 D r multiply-adds per element (the padding of a
rank to a multiple of 4 not counted), `expand_tflops` the same work over the time of the D expansions alone.
"""
import argparse
import json
import os

from mx8sum_bench import ROOT, load_pkg, timed_alternately


def bench_rounds(fa, torch, np, mats, side, clients, ranks, reps, warmup):
    table, n = fa.lowrank_mats([(side, side)] * mats)
    plan = torch.from_numpy(fa.lowrank_plan(table, n)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    g = torch.rand(n, device="cuda", generator=gen) * 2 - 1
    out_e, out_s = torch.empty_like(g), torch.empty_like(g)
    Dmax = max(clients)
    slots = [torch.empty_like(g) for _ in range(Dmax)]
    res = {"n": n, "mats": mats, "side": side, "rounds": []}
    for r in ranks:
        flen = fa.lowrank_len(table, n, r)
        f = [(torch.rand(flen, device="cuda", generator=gen) * 2 - 1) / 8 for _ in range(Dmax)]
        for D in clients:
            w = np.full(D, 1.0 / D, np.float32)

            def expansions():
                for c in range(D):
                    fa.lowrank_expand_device(plan, f[c], r, n, slots[c], ref=g)

            def expanded():
                expansions()
                fa.reduce_device(slots[:D], w, n, fa.F32, out_e)

            def summed():
                fa.lowrank_sum_device(plan, f[:D], [r] * D, n, out_s, weights=w, ref=g)

            t = timed_alternately(torch, {"expanded": expanded, "sum": summed, "expansions": expansions}, reps, warmup)
            err = float((out_e - out_s).abs().max())  # not the same bits (fa.h rule 5): D + 1 roundings against one
            assert err < 1e-4, err
            flop = 2.0 * D * r * n
            t.update(D=D, r=r, expanded_bytes=(12 * D + 4) * n, sum_bytes=8 * n, max_abs_diff=err,
                     ratio=t["sum"]["median_ms"] / t["expanded"]["median_ms"], byte_model_ratio=8 / (12 * D + 4),
                     sum_tflops=flop / t["sum"]["median_ms"] / 1e9, expand_tflops=flop / t["expansions"]["median_ms"] / 1e9,
                     sum_tb_s=8 * n / t["sum"]["median_ms"] / 1e9)
            res["rounds"].append(t)
            print("r %d D %d" % (r, D), {s: (round(t[s]["median_ms"], 3), round(t[s]["min_ms"], 3), round(t[s]["max_ms"], 3))
                                         for s in ("expanded", "sum", "expansions")},
                  "ratio %.3f (bytes %.3f) Tflop/s %.1f vs %.1f TB/s %.2f"
                  % (t["ratio"], t["byte_model_ratio"], t["sum_tflops"], t["expand_tflops"], t["sum_tb_s"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowranksum_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clients", default="8,32,64")
    ap.add_argument("--ranks", default="4,16,64")
    ap.add_argument("--mats", type=int, default=64)
    ap.add_argument("--side", type=int, default=1024)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "lowranksum_bench.py needs a GPU"
    fa = load_pkg()
    ints = lambda s: [int(x) for x in s.split(",")]
    res = bench_rounds(fa, torch, np, a.mats, a.side, ints(a.clients), ints(a.ranks), a.reps, a.warmup)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
