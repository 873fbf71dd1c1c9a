#!/usr/bin/env python3
"""Times the clip stage's norm pass against the FedAvg chain of a reference build of the library, and a clipped
round against a plain one, on the north-star shape (D = 32 clients x 256 MiB fp32).

    tools/clip_bench.py --parent-lib PATH/libfa.so [--out profiles/clip_bench.json] [--reps 15] [--warmup 3]

--parent-lib is a libfa.so built from the commit before the clip stage: its fa_reduce_device over the same 32
device buffers is the yardstick (the norm pass reads (D + 1) / D of the chain's input and writes nothing).  The
two are timed alternately, one launch each per repetition, with HIP events on one stream, and compared by their
medians.  The norm pass is timed as the library runs it: fa_clip_sumsq_device on a context (the sums kernel,
the kernel that adds the partials, the read-back of the D sums).

The second part times whole device-resident rounds through a context, again alternately: fa_reduce_part of a
plain part and of a clipped one whose 32 clients are all scaled down (so the reference joins the chain as its
first term), host clock around the call and the wait for it.  The clipped round is the norm pass, the host's
wait for its sums, the chain over D + 1 buffers and the copy of the output into the reference.
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


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=N)
    args = ap.parse_args()
    import numpy as np
    import torch
    fa = load_pkg()
    fa.lib()
    n = args.n
    P, I, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.fa_reduce_device.restype = I
    parent.fa_reduce_device.argtypes = [P, I, P, P, I, S, I, P, I, I, P, P]
    assert not hasattr(parent, "fa_set_clip"), "--parent-lib already has the clip stage"

    clients = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(D)]
    for k, c in enumerate(clients):
        fa.fill_uniform(c, n, fa.F32, 0xC11F, k)
    ref = torch.zeros(n, dtype=torch.float32, device="cuda")
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    arr = (ctypes.c_void_p * D)(*[c.data_ptr() for c in clients])
    w = np.full(D, 1.0 / D, np.float32)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    result = {"D": D, "n": n, "reps": args.reps, "warmup": args.warmup}

    with fa.Aggregator(1) as agg:
        def chain():
            rc = parent.fa_reduce_device(None, 0, arr, w.ctypes.data, D, n, fa.F32, out.data_ptr(), fa.F32, fa.FEDAVG,
                                         None, h)
            assert rc == 0, rc

        def norm():
            return fa.clip_sumsq_device(clients, n, fa.F32, ref, stream=h, ctx=agg)

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        t_chain, t_norm = [], []
        for i in range(args.warmup + args.reps):
            c, q = event_ms(chain), event_ms(norm)
            if i >= args.warmup:
                t_chain.append(c)
                t_norm.append(q)
        q = norm()
        result.update({"parent_chain_ms": t_chain, "norm_pass_ms": t_norm,
                       "parent_chain_median_ms": statistics.median(t_chain),
                       "norm_pass_median_ms": statistics.median(t_norm),
                       "norm_over_chain": statistics.median(t_norm) / statistics.median(t_chain),
                       "norm_bytes": (D + 1) * 4 * n, "chain_bytes": (D + 1) * 4 * n,
                       "norm_GBps": (D + 1) * 4 * n / statistics.median(t_norm) / 1e6,
                       "sumsq_first": float(q[0]), "sumsq_expected_about": n / 3.0})
    del clients, out, ref
    torch.cuda.empty_cache()

    # whole device-resident rounds: a plain part and a clipped one, alternately
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_clip(1000.0, 2)  # every client is sqrt(n / 3) from the zero reference: all scaled down
        for part in (1, 2):
            for k in range(D):
                ptr, cnt, _ = agg.slot(part, 0, k)
                fa.fill_uniform(ptr, cnt, fa.F32, 0xC11F, k)
                agg.submit_commit(part, k, 1.0 / D)
        torch.cuda.synchronize()

        def round_ms(part):
            if part == 2:  # the reference the round before left is the aggregate itself: start from zeros again
                agg.set_clip_reference(2, zeros)
            t0 = time.perf_counter()
            agg.reduce(part)
            agg.sync()
            return (time.perf_counter() - t0) * 1e3

        zeros = np.zeros(n, np.float32)
        t_plain, t_clip = [], []
        for i in range(args.warmup + args.reps):
            a, b = round_ms(1), round_ms(2)
            if i >= args.warmup:
                t_plain.append(a)
                t_clip.append(b)
        Q, scales, included, n_clipped = agg.clip_round(2)
        result.update({"plain_round_ms": t_plain, "clipped_round_ms": t_clip,
                       "plain_round_median_ms": statistics.median(t_plain),
                       "clipped_round_median_ms": statistics.median(t_clip),
                       "clipped_over_plain": statistics.median(t_clip) / statistics.median(t_plain),
                       "clipped_clients": int(n_clipped)})
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
