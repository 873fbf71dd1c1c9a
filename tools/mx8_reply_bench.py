#!/usr/bin/env python3
"""Times MX8 replies (fa.h "MX8 replies"): the encoder kernel against the expansion kernel and against the D2H of the
codes it precedes, and the host-inclusive round that ends in fa_finalize_mx8 against the one that ends in
fa_finalize_gather.

    tools/mx8_reply_bench.py --parent-lib PATH/libfa.so [--out profiles/mx8_reply_bench.json] [--reps 7] [--warmup 2]

--parent-lib is a libfa.so built from the commit before MX8 replies; it runs on a context of its own.  One session,
one GPU; the sides of a comparison are timed alternately, one round each per repetition, and compared by their medians
with min and max kept.

The kernel alone, at n = 64 Mi in f32 and bf16, between two events on one stream:
  raw     fa_mx8_encode_device with the output on the sent model: 8 bytes read, 5 + 1/32 written per f32 element;
  stage   the stage's own launch, which writes g' twice (the part's output and the sent model): 17 + 1/32 bytes per f32
          element, 9 + 1/32 per 16-bit one.  It has no entry of its own, so it is timed as the difference of
          fa_reduce_part over one client with the stage on and off (the same chain launch before it);
  expand  fa_mx8_expand_device, f32 against f32, 9 + 1/32 bytes per element: the rate the encoder is set beside;
  d2h     the copy of the n + n / 32 code bytes into pinned memory.

Host-inclusive round, at the north star's shape (D = 32 x 64 Mi fp32) and C2's (D = 8 x 12.6 M fp32): D pinned MX8
receipts submitted, then the finalize into pinned memory, host clock around the whole.
  (i)   the parent's round with fa_finalize_gather;
  (ii)  this library's round with the reply stage on and fa_finalize_mx8;
  (iii) this library's round as (i), the stage off -- the unchanged path.
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
MI = 1024 * 1024
SHAPES = [("north_star", 32, 64 * MI), ("c2", 8, 12_557_962)]
KERNEL_N = 64 * MI
NBUF = 4
P, I, S, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
FA_F32, FA_BF16, FA_FEDAVG, FA_HOST_PINNED = 0, 1, 0, 1


def load_pkg():
    spec = importlib.util.spec_from_file_location("mhfsl_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mhfsl_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "ms": ts}


def spread(ts):
    return max(ts) - min(ts)


def declare(lib):
    for name, res, args in (("fa_create", I, [ctypes.POINTER(P), I, I]), ("fa_destroy", None, [P]),
                            ("fa_bucket_define", I, [P, I, S, I, I, I, I]), ("fa_set_mx8", I, [P, I, I]),
                            ("fa_mx8_set_reference", I, [P, I, P]), ("fa_submit_mx8", I, [P, I, I, P, P, F, I]),
                            ("fa_finalize_gather", I, [P, I, I, P, P, I]), ("fa_last_error", ctypes.c_char_p, [])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Side:
    """One library's context with one fp32 part of D x n that takes MX8 receipts, driven through the C ABI alone."""

    def __init__(self, lib, D, n, reference, reply=False):
        self.lib, self.D, self.n, self.reply = lib, D, n, reply
        self.ctx = P()
        self.ok(lib.fa_create(ctypes.byref(self.ctx), 1, 0))
        self.ok(lib.fa_bucket_define(self.ctx, 1, n, FA_F32, FA_F32, D, FA_FEDAVG))
        self.ok(lib.fa_set_mx8(self.ctx, 1, 1))
        if reply:
            self.ok(lib.fa_set_mx8_reply(self.ctx, 1, 1))
        self.ok(lib.fa_mx8_set_reference(self.ctx, 1, reference.ctypes.data))  # the model the owners hold

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.fa_last_error().decode())

    def round(self, qs, es, dst, q_out, e_out):
        t0 = time.perf_counter()
        for k in range(self.D):
            self.ok(self.lib.fa_submit_mx8(self.ctx, 1, k, qs[k % len(qs)].ctypes.data, es[k % len(es)].ctypes.data,
                                           1.0 / self.D, FA_HOST_PINNED))
        if self.reply:
            self.ok(self.lib.fa_finalize_mx8(self.ctx, 1, q_out.ctypes.data, e_out.ctypes.data, FA_HOST_PINNED))
        else:
            ptrs, sizes = (P * 1)(dst.ctypes.data), (S * 1)(dst.nbytes)
            self.ok(self.lib.fa_finalize_gather(self.ctx, 1, 1, ptrs, sizes, FA_HOST_PINNED))
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.lib.fa_destroy(self.ctx)


def bench_rounds(fa, parent, np, D, n, reps, warmup):
    rng = np.random.default_rng(D)
    nb = fa.mx8_scale_bytes(n)
    pins, qs, es = [], [], []
    for b in range(NBUF):
        pq, pe = fa.PinnedBuffer(n), fa.PinnedBuffer(nb)
        pins += [pq, pe]
        q, e = pq.view(np.int8), pe.view(np.uint8)
        q[:] = np.resize(np.roll(rng.integers(-127, 128, 1 << 20).astype(np.int8), b * 4099), n)
        e[:] = np.resize(rng.integers(120, 128, 1 << 16).astype(np.uint8), e.size)
        qs.append(q)
        es.append(e)
    pdst, pq_out, pe_out = fa.PinnedBuffer(4 * n), fa.PinnedBuffer(n), fa.PinnedBuffer(nb)
    pins += [pdst, pq_out, pe_out]
    dst, q_out, e_out = pdst.view(np.float32), pq_out.view(np.int8), pe_out.view(np.uint8)
    dst[:] = np.resize(rng.uniform(-1, 1, 1 << 20).astype(np.float32), n)  # the reference of every side
    L = fa.lib()
    old, new_reply, new_plain = Side(parent, D, n, dst), Side(L, D, n, dst, reply=True), Side(L, D, n, dst)
    t = {"parent_gather": [], "reply_mx8": [], "gather": []}
    for i in range(warmup + reps):
        a = old.round(qs, es, dst, q_out, e_out)
        b = new_reply.round(qs, es, dst, q_out, e_out)
        c = new_plain.round(qs, es, dst, q_out, e_out)
        if i >= warmup:
            t["parent_gather"].append(a)
            t["reply_mx8"].append(b)
            t["gather"].append(c)
    assert np.isfinite(dst[:4096]).all() and q_out[:1 << 20].any()
    nan = ctypes.c_uint64()
    new_reply.ok(L.fa_mx8_reply_stats(new_reply.ctx, 1, ctypes.byref(nan)))
    for s in (old, new_reply, new_plain):
        s.close()
    for p in pins:
        p.close()
    m = {k: statistics.median(v) for k, v in t.items()}
    return {"D": D, "n": n, "parent_gather_round": summary(t["parent_gather"]), "reply_mx8_round": summary(t["reply_mx8"]),
            "gather_round": summary(t["gather"]), "reply_mx8_over_parent": m["reply_mx8"] / m["parent_gather"],
            "gather_over_parent": m["gather"] / m["parent_gather"], "d2h_bytes_saved": 4 * n - n - nb,
            "reply_mx8_below_parent_by_more_than_both_spreads":
                m["parent_gather"] - m["reply_mx8"] > spread(t["parent_gather"]) + spread(t["reply_mx8"]),
            "gather_within_spreads_of_parent":
                abs(m["gather"] - m["parent_gather"]) <= spread(t["parent_gather"]) + spread(t["gather"]),
            "nan_blocks": nan.value}


def bench_kernel(fa, torch, np, n, reps, warmup):
    nb = fa.mx8_scale_bytes(n)
    stream = torch.cuda.Stream()
    L = fa.lib()

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    out = {"n": n}
    q = torch.empty(n, dtype=torch.int8, device="cuda")
    e = torch.empty(nb, dtype=torch.uint8, device="cuda")
    host = torch.empty(n + nb, dtype=torch.uint8).pin_memory()
    dev = torch.empty(n + nb, dtype=torch.uint8, device="cuda")
    g32 = torch.rand(n, dtype=torch.float32, device="cuda")
    x32 = torch.empty(n, dtype=torch.float32, device="cuda")
    eq = torch.randint(-127, 128, (n,), dtype=torch.int8, device="cuda")
    ee = torch.randint(120, 128, (nb,), dtype=torch.uint8, device="cuda")

    def expand():
        fa.mx8_expand_device(eq, ee, n, x32, fa.F32, ref=g32, ref_dtype=fa.F32, stream=stream.cuda_stream)

    def d2h():
        with torch.cuda.stream(stream):
            host.copy_(dev, non_blocking=True)

    for name, tdt, fdt, es in (("f32", torch.float32, fa.F32, 4), ("bf16", torch.bfloat16, fa.BF16, 2)):
        sent = (torch.rand(n, dtype=torch.float32, device="cuda") * 2 - 1).to(tdt)
        new = (sent.float() + 0.01 * torch.randn(n, dtype=torch.float32, device="cuda")).to(tdt)
        keep = sent.clone()

        def raw():
            fa.mx8_encode_device(new, sent, n, q, e, out=sent, dtype=fdt, stream=stream.cuda_stream)

        # the stage's launch: one client, weight 1, reduced on `stream` with the stage on and off
        sides = {}
        host_model = keep.float().cpu().numpy() if es == 4 else keep.view(torch.int16).cpu().numpy().view(np.uint16)
        host_new = new.float().cpu().numpy() if es == 4 else new.view(torch.int16).cpu().numpy().view(np.uint16)
        for on in (True, False):
            agg = fa.Aggregator(1)
            agg.define(1, n, fdt, fdt, 1)
            if on:
                agg.set_mx8_reply(True, 1)
                agg.set_mx8_reference(1, host_model)
            agg.submit(1, 0, host_new, 1.0)
            agg.sync()
            sides[on] = agg
        t = {"raw": [], "on": [], "off": [], "expand": [], "d2h": []}
        for i in range(warmup + reps):
            sent.copy_(keep)
            torch.cuda.synchronize()
            r = {"raw": event_ms(raw),
                 "on": event_ms(lambda: sides[True].reduce(1, stream=stream.cuda_stream)),
                 "off": event_ms(lambda: sides[False].reduce(1, stream=stream.cuda_stream))}
            if es == 4:
                r["expand"], r["d2h"] = event_ms(expand), event_ms(d2h)
            if i >= warmup:
                for k, v in r.items():
                    t[k].append(v)
        for agg in sides.values():
            agg.close()
        stage = [a - b for a, b in zip(t["on"], t["off"])]
        raw_bytes, stage_bytes = n * (2 * es + es + 1) + nb, n * (2 * es + 2 * es + 1) + nb
        res = {"raw": summary(t["raw"]), "raw_bytes": raw_bytes, "raw_GBps": raw_bytes / statistics.median(t["raw"]) / 1e6,
               "reduce_stage_on": summary(t["on"]), "reduce_stage_off": summary(t["off"]), "stage": summary(stage),
               "stage_bytes": stage_bytes, "stage_GBps": stage_bytes / statistics.median(stage) / 1e6}
        if es == 4:
            exp_bytes = n + nb + 8 * n
            me, mc = statistics.median(t["expand"]), statistics.median(t["d2h"])
            res.update({"expand": summary(t["expand"]), "expand_GBps": exp_bytes / me / 1e6,
                        "d2h_of_codes": summary(t["d2h"]), "d2h_GiBps": (n + nb) / mc / 1e-3 / 2 ** 30,
                        "stage_over_d2h": statistics.median(stage) / mc, "raw_over_d2h": statistics.median(t["raw"]) / mc,
                        "stage_rate_over_expand_rate": res["stage_GBps"] / (exp_bytes / me / 1e6),
                        "raw_rate_over_expand_rate": res["raw_GBps"] / (exp_bytes / me / 1e6)})
            out["d2h_median_ms"] = mc
        else:
            res["stage_over_d2h"] = statistics.median(stage) / out["d2h_median_ms"]
        out[name] = res
        del sent, new, keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="north_star,c2")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("mx8_reply_bench: no GPU (nothing is measured without one)")
    fa = load_pkg()
    fa.lib()
    parent = declare(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    assert not hasattr(parent, "fa_set_mx8_reply"), "--parent-lib already has MX8 replies"
    L = declare(fa.lib())
    for name, res, a in (("fa_set_mx8_reply", I, [P, I, I]), ("fa_finalize_mx8", I, [P, I, P, P, I]),
                         ("fa_mx8_reply_stats", I, [P, I, P])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, a
    result = {"reps": args.reps, "warmup": args.warmup}

    def brief(d):
        return {k: (v if not isinstance(v, dict) else brief({a: b for a, b in v.items() if a != "ms"})) for k, v in d.items()}

    result["kernel"] = bench_kernel(fa, torch, np, KERNEL_N, args.reps, args.warmup)
    print(json.dumps({"kernel": brief(result["kernel"])}), flush=True)
    for name, D, n in SHAPES:
        if name not in args.shapes.split(","):
            continue
        result[name] = bench_rounds(fa, parent, np, D, n, args.reps, args.warmup)
        print(json.dumps({name: brief(result[name])}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
