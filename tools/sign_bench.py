#!/usr/bin/env python3
"""Times the sign-vote stage (fa.h "Sign-vote stage") on the GPU.

    tools/sign_bench.py [--out profiles/sign_bench.json] [--reps 7] [--warmup 2]

Two shapes, f32, the majority rule without planes: the north star (D = 32, n = 64 Mi) and C2's (D = 8, n = 12,557,962).
Per shape, through one context:
  kernel          device-resident rounds, fa_reduce_part on one stream between two HIP events, alternately the vote
                  over the D shadows (a relative round: g is the part's output) and a plain FA_FEDAVG part's chain at
                  the same D and n.  The vote's bytes per second count the D / 8 + 8 bytes per element it must move.
  host-inclusive  host clock around D pinned submits and a pinned finalize, alternately sign receipts and rot1
                  receipts (rot1's pinned submit path: its H2D and expansion, then the ordinary chain).
Comparison figures, not targets; the mean rule, 16-bit types, planes and more than one GPU are not measured here.
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
SHAPES = {"north_star": (32, 64 * 1024 * 1024), "c2": (8, 12_557_962)}


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def alternate(runs, reps, warmup):
    ts = {k: [] for k in runs}
    for i in range(warmup + reps):
        for k, fn in runs.items():
            t = fn()
            if i >= warmup:
                ts[k].append(t)
    return {k: spread(v) for k, v in ts.items()}


def shape(fa, torch, np, D, n, reps, warmup):
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(D)
    words, blocks = fa.sign_words(n), fa.rot1_blocks(n)
    pin_sign, pin_rot, pin_out = fa.PinnedBuffer(D * words * 4), fa.PinnedBuffer(D * blocks * 516), fa.PinnedBuffer(n * 4)
    sign = [pin_sign.view(np.uint32, words, k * words * 4) for k in range(D)]
    rot = [(pin_rot.view(np.uint32, blocks * 128, k * blocks * 516), pin_rot.view(np.float32, blocks, k * blocks * 516 + blocks * 512))
           for k in range(D)]
    for k in range(D):
        sign[k][:] = rng.integers(0, 2 ** 32, words, dtype=np.uint32)
        rot[k][0][:] = rng.integers(0, 2 ** 32, blocks * 128, dtype=np.uint32)
        rot[k][1][:] = 1e-3
    out = pin_out.view(np.float32, n)
    res = {"D": D, "n": n, "vote_bytes_per_element": D / 8 + 8, "chain_bytes_per_element": 4 * D + 4}
    with fa.Aggregator(1) as agg:
        for part in (1, 2, 3):
            agg.define(part, n, fa.F32, fa.F32, D)
        agg.set_sign(2, 1e-3)
        agg.set_rot1(True, 3)
        agg.set_mx8_reference(2, np.zeros(n, np.float32))
        agg.set_mx8_reference(3, np.zeros(n, np.float32))
        for k in range(D):
            ptr, cnt, _ = agg.slot(1, 0, k)
            fa.fill_uniform(ptr, cnt, fa.F32, 0x51, k)
            agg.submit_commit(1, k, 1.0 / D)
            agg.submit_sign(2, k, sign[k], pinned=True)
        torch.cuda.synchronize()

        def event_ms(part):
            def run():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                agg.reduce(part, stream=stream)
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b)
            return run

        res["kernel"] = alternate({"vote": event_ms(2), "plain_chain": event_ms(1)}, reps, warmup)
        agg.finalize_gather(2, [out], pinned=True)  # ends the device-resident round

        def host_ms(part, submit):
            def run():
                t0 = time.perf_counter()
                for k in range(D):
                    submit(part, k)
                agg.finalize_gather(part, [out], pinned=True)
                return (time.perf_counter() - t0) * 1e3
            return run

        res["host_inclusive"] = alternate({
            "vote": host_ms(2, lambda p, k: agg.submit_sign(p, k, sign[k], pinned=True)),
            "rot1": host_ms(3, lambda p, k: agg.submit_rot1(p, k, rot[k][0], rot[k][1], 0x51 + k, 1.0 / D, pinned=True)),
        }, reps, warmup)
    vote_s = res["kernel"]["vote"]["median_ms"] * 1e-3
    res["vote_bytes_per_s"] = n * (D / 8 + 8) / vote_s
    res["chain_bytes_per_s"] = n * (4 * D + 4) / (res["kernel"]["plain_chain"]["median_ms"] * 1e-3)
    res["chain_over_vote"] = res["kernel"]["plain_chain"]["median_ms"] / res["kernel"]["vote"]["median_ms"]
    for b in (pin_sign, pin_rot, pin_out):
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "sign_bench needs a GPU"
    fa = load_pkg()
    fa.lib()
    result = {"reps": args.reps, "warmup": args.warmup}
    for name, (D, n) in SHAPES.items():
        result[name] = shape(fa, torch, np, D, n, args.reps, args.warmup)
        torch.cuda.empty_cache()

    def brief(v):
        return {k: brief(x) for k, x in v.items() if k != "ms"} if isinstance(v, dict) else v
    print(json.dumps(brief(result)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
