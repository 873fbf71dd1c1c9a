#!/usr/bin/env python3
"""Times a sparse-sum round (fa.h "Sparse-sum stage") beside the route it replaces, on the same commit.

    tools/sparse_bench.py [--out profiles/sparse_bench.json] [--reps 7] [--warmup 2] [--clients 8,32,64] [--skip-c2]

One session, one GPU; the sides of a comparison are timed alternately, one round each per repetition, and compared by
their medians with min and max kept.

Device rounds, at n = 64 Mi fp32, D in {8, 32, 64} owners of k ~ n / 1000, n / 100, n / 10 entries each (a Bernoulli
draw per element, so k varies a little around its mean), between two events on one stream:
  expanded  D calls of fa_topk_expand_device into D dense slots, then fa_reduce_device over them: what fa_submit_topk
            and the chain enqueue;
  sparse    one fa_sparse_sum_device (the cut pass and the accumulate pass), with the tile the host takes by itself;
  small, big  the same call with the tile forced, so that the host's choice rests on numbers.
Within a repetition the order is expanded, sparse, small, big: `sparse` follows the expanded round's tens of GB and may
read a little slower than the same kernel forced (`small` or `big`) right after it.  `ratio` is sparse / expanded.
The two routes weigh the reference differently (fa.h rule 3): the bench gives weights of sum one and compares times only.
Byte models, per round: expanded (12 D + 4) n, sparse 8 sum k + 8 n + the cut table.
Host-inclusive, at C2's shape (12.6 M fp32 elements), D = 8 owners of k = n / 100 from pinned memory through a context:
host clock from the first submit to fa_sync after the reducing call, a part with fa_set_topk beside one with
fa_set_sparse_sum.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "multihop-federeated-split-learning_amd")
MI = 1024 * 1024
KERNEL_N, C2_N, C2_D = 64 * MI, 12_557_962, 8


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


def bench_rounds(fa, torch, np, clients, reps, warmup):
    n = KERNEL_N
    gen = torch.Generator(device="cuda").manual_seed(1)
    g = torch.rand(n, device="cuda", generator=gen) * 2 - 1
    out_e, out_s = torch.empty_like(g), torch.empty_like(g)
    Dmax = max(clients)
    slots = [torch.empty_like(g) for _ in range(Dmax)]
    work = torch.empty(fa.sparse_sum_workspace(n, Dmax), dtype=torch.uint8, device="cuda")
    res = {"n": n, "rounds": []}
    for frac in (1000, 100, 10):
        idx, val = [], []
        for c in range(Dmax):  # ascending by construction
            i = torch.nonzero(torch.rand(n, device="cuda", generator=gen) < 1.0 / frac).flatten().to(torch.int32)
            idx.append(i)
            val.append(torch.randn(i.numel(), device="cuda", generator=gen))
        for D in clients:
            k = [int(i.numel()) for i in idx[:D]]
            w = np.full(D, 1.0 / D, np.float32)

            def expanded():
                for c in range(D):
                    fa.topk_expand_device(idx[c], val[c], k[c], n, slots[c], ref=g)
                fa.reduce_device(slots[:D], w, n, fa.F32, out_e)

            def sparse(tile=None):
                fa.sparse_sum_device(idx[:D], val[:D], k, n, out_s, work, weights=w, ref=g, tile=tile)

            r = timed_alternately(torch, {"expanded": expanded, "sparse": sparse, "small": lambda: sparse(0),
                                          "big": lambda: sparse(1)}, reps, warmup)
            # the two routes agree up to their roundings (they are not the same bits: fa.h rule 3)
            err = float((out_e - out_s).abs().max())
            assert err < 1e-4, err
            form = fa.sparse_sum_form(n, k, out_s, fa.F32, g, fa.F32)
            r.update(D=D, k_mean=sum(k) / D, density=sum(k) / (D * n), big_tile=bool(form & fa.SPARSE_BIG_TILE),
                     expanded_bytes=(12 * D + 4) * n, sparse_bytes=8 * sum(k) + 8 * n, max_abs_diff=err,
                     ratio=r["sparse"]["median_ms"] / r["expanded"]["median_ms"])
            r["sparse_tb_s"] = r["sparse_bytes"] / r["sparse"]["median_ms"] / 1e9
            r["expanded_tb_s"] = r["expanded_bytes"] / r["expanded"]["median_ms"] / 1e9
            res["rounds"].append(r)
            print("n/%d D %d" % (frac, D), {s: (round(r[s]["median_ms"], 3), round(r[s]["min_ms"], 3), round(r[s]["max_ms"], 3))
                                            for s in ("expanded", "sparse", "small", "big")},
                  "ratio %.3f big %s TB/s %.2f vs %.2f" % (r["ratio"], r["big_tile"], r["sparse_tb_s"], r["expanded_tb_s"]), flush=True)
    return res


def bench_c2(fa, np, reps, warmup):
    n, D, k = C2_N, C2_D, C2_N // 100
    rng = np.random.default_rng(2)
    pins, idx, val = [], [], []
    for c in range(D):
        pi, pv = fa.PinnedBuffer(4 * k), fa.PinnedBuffer(4 * k)
        pins += [pi, pv]
        idx.append(pi.view(np.uint32))
        val.append(pv.view(np.float32))
        idx[c][:] = np.sort(rng.choice(n, k, replace=False))
        val[c][:] = rng.standard_normal(k).astype(np.float32)
    x = np.resize(rng.uniform(-1, 1, 1 << 20).astype(np.float32), n)
    t = {"topk_round": [], "sparse_round": []}
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_topk(k, 1)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_sparse_sum(2, k)
        for part in (1, 2):
            agg.set_mx8_reference(part, x)
        for i in range(warmup + reps):
            for name, part, submit in (("topk_round", 1, agg.submit_topk), ("sparse_round", 2, agg.submit_sparse)):
                t0 = time.perf_counter()
                for c in range(D):
                    submit(part, c, idx[c], val[c], 1.0 / D, pinned=True)
                agg.reduce(part)
                agg.sync()
                if i >= warmup:
                    t[name].append((time.perf_counter() - t0) * 1e3)
    for p in pins:
        p.close()
    r = {name: summary(v) for name, v in t.items()}
    r.update(n=n, D=D, k=k, ratio=r["sparse_round"]["median_ms"] / r["topk_round"]["median_ms"])
    print("C2", {s: (round(r[s]["median_ms"], 3), round(r[s]["min_ms"], 3), round(r[s]["max_ms"], 3))
                 for s in ("topk_round", "sparse_round")}, "ratio %.3f" % r["ratio"], flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clients", default="8,32,64")
    ap.add_argument("--skip-c2", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "sparse_bench.py needs a GPU"
    fa = load_pkg()
    res = {"rounds": bench_rounds(fa, torch, np, [int(d) for d in a.clients.split(",")], a.reps, a.warmup)}
    if not a.skip_c2:
        res["c2"] = bench_c2(fa, np, a.reps, a.warmup)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
