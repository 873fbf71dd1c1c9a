"""MI355X FedAvg aggregation path -- Python view of the C ABI in include/fedavg/fa.h.

The product is ``lib/libfa.so`` (HIP kernels + C ABI, built by this directory's
Makefile).  This module only binds it with ctypes so tests, bench.py and the
multi-GPU driver (``shard.py``) can call it; there is no CPU fallback: if the
library or a gfx950 device is missing, calls raise ``FaError``.

Names mirror the reference aggregator (pipeline_simulation/aggregator.cpp):
a *part* is one model part bucket (``model_part`` 1 = parts[0].layers[0],
m >= 2 = parts[1].layers[m-2]), a *client slot* is one data owner's receipt.
"""
import ctypes
import os
import threading

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libfa.so")

F32, BF16, F16 = 0, 1, 2  # F16: IEEE binary16 (torch.float16 / np.float16)
FEDAVG, LITERAL, TRIMMED = 0, 1, 2
TRIM_MEDIAN = -1  # FA_TRIM_MEDIAN: the largest valid trim, (D-1)/2
TRIMMED_MAX_CLIENTS = 128
KRUM_MAX_CLIENTS = 128  # FA_KRUM_MAX_CLIENTS: the Krum stage and pairdist_device
GEOMED_MAX_CLIENTS, GEOMED_MAX_ITERS = 128, 64  # FA_GEOMED_MAX_*: the geomed stage and geomed_pass_device
# fa_opt_rule: the server-optimizer stage (FedAvgM, FedAdagrad, FedAdam, FedYogi; fa.h "Server optimizer")
OPT_NONE, OPT_MOMENTUM, OPT_ADAGRAD, OPT_ADAM, OPT_YOGI = 0, 1, 2, 3, 4
SHARD_RANGE, SHARD_CLIENT_RS, ACCUMULATE_ON_ARRIVAL, TEST_SHARED_DEVICE = 0x1, 0x2, 0x4, 0x100
OK, ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_STATE, ERR_NODEV, ERR_ALIGN, ERR_NCCL = 0, -1, -2, -3, -4, -5, -6, -7
DTYPE_SIZE = {F32: 4, BF16: 2, F16: 2}
# host view of a reduced bucket: numpy has no bf16, so a bf16 output comes back as its uint16 bits
_OUT_NP = {F32: np.float32, BF16: np.uint16, F16: np.float16}

_lib = None


class FaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fa error %d: %s" % (code, msg))
        self.code = code


class _Tuning(ctypes.Structure):
    _fields_ = [("block", ctypes.c_int), ("max_blocks", ctypes.c_int), ("unroll", ctypes.c_int),
                ("load_policy", ctypes.c_int), ("store_policy", ctypes.c_int), ("slot_skew", ctypes.c_int),
                ("walk", ctypes.c_int), ("rs_chunks", ctypes.c_int), ("piece_span_kib", ctypes.c_int),
                ("piece_split_kib", ctypes.c_int)]


class _ServerOpt(ctypes.Structure):
    _fields_ = [("rule", ctypes.c_int), ("lr", ctypes.c_float), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("tau", ctypes.c_float)]


def build():
    """Compile libfa.so in-tree (hipcc, gfx950)."""
    import subprocess
    subprocess.run(["make", "-C", PKG_DIR, "-j8"], check=True)
    return LIB_PATH


def lib():
    """Load libfa.so (torch, when used, must be imported first: both share libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FaError(ERR_NODEV, "libfa.so not built at %s (run make -C %s)" % (LIB_PATH, PKG_DIR))
    L = ctypes.CDLL(LIB_PATH)
    P, S, I, F, U64, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32
    sig = {
        "fa_version": (I, []),
        "fa_last_error": (ctypes.c_char_p, []),
        "fa_device_count": (I, [ctypes.POINTER(I)]),
        "fa_create": (I, [ctypes.POINTER(P), I, I]),
        "fa_create_ex": (I, [ctypes.POINTER(P), ctypes.POINTER(I), I, I]),
        "fa_reduce_part": (I, [P, I, P, P]),
        "fa_bucket_slot": (I, [P, I, I, I, ctypes.POINTER(P), ctypes.POINTER(S), ctypes.POINTER(S)]),
        "fa_bucket_pieces": (I, [P, I, I, ctypes.POINTER(I)]),
        "fa_bucket_piece": (I, [P, I, I, I, I, ctypes.POINTER(P), ctypes.POINTER(S), ctypes.POINTER(S)]),
        "fa_bucket_output": (I, [P, I, I, ctypes.POINTER(P)]),
        "fa_sync": (I, [P]),
        "fa_copy_output": (I, [P, I, P]),
        "fa_destroy": (None, [P]),
        "fa_bucket_define": (I, [P, I, S, I, I, I, I]),
        "fa_set_literal_divisor": (I, [P, I, F]),
        "fa_set_trim": (I, [P, I, I]),
        "fa_trimmed_device": (I, [P, I, P, I, S, I, P, I, I, P]),
        "fa_set_server_opt": (I, [P, I, ctypes.POINTER(_ServerOpt)]),
        "fa_get_server_opt": (I, [P, I, ctypes.POINTER(_ServerOpt)]),
        "fa_server_opt_set_state": (I, [P, I, P, P, P, U64]),
        "fa_server_opt_get_state": (I, [P, I, P, P, P, ctypes.POINTER(U64)]),
        "fa_server_opt_device": (I, [P, I, ctypes.POINTER(_ServerOpt), P, P, P, P, S, P, I, P]),
        "fa_set_clip": (I, [P, I, F]),
        "fa_clip_set_reference": (I, [P, I, P]),
        "fa_clip_get_reference": (I, [P, I, P]),
        "fa_clip_get_round": (I, [P, I, P, P, P, ctypes.POINTER(I)]),
        "fa_clip_scale": (F, [ctypes.c_double, F, ctypes.POINTER(I)]),
        "fa_clip_sumsq_device": (I, [P, I, P, I, S, I, P, P, P]),
        "fa_set_krum": (I, [P, I, I, I]),
        "fa_krum_get_round": (I, [P, I, P, P, P, ctypes.POINTER(I)]),
        "fa_krum_select": (I, [P, I, I, I, P, P, ctypes.POINTER(I)]),
        "fa_krum_weights": (I, [P, P, I, P]),
        "fa_pairdist_device": (I, [P, I, P, I, S, I, P, P]),
        "fa_set_geomed": (I, [P, I, I, F]),
        "fa_get_geomed": (I, [P, I, ctypes.POINTER(I), ctypes.POINTER(F)]),
        "fa_geomed_get_round": (I, [P, I, ctypes.POINTER(I), P, P, P, P]),
        "fa_geomed_weights": (I, [P, P, P, I, F, P]),
        "fa_geomed_pass_device": (I, [P, I, P, P, I, S, I, P, P, P, P]),
        "fa_set_bulyan": (I, [P, I, I]),
        "fa_bulyan_get_round": (I, [P, I, P, P, P, P, ctypes.POINTER(I)]),
        "fa_bulyan_select": (I, [P, I, I, P, P, P, ctypes.POINTER(I)]),
        "fa_centered_device": (I, [P, I, P, I, S, I, P, I, I, P]),
        "fa_set_noise": (I, [P, I, F, U64]),
        "fa_get_noise": (I, [P, I, ctypes.POINTER(F), ctypes.POINTER(U64)]),
        "fa_noise_get_round": (I, [P, I, ctypes.POINTER(U64)]),
        "fa_noise_set_round": (I, [P, I, U64]),
        "fa_noise_device": (I, [P, I, P, S, P, I, F, U64, U32, U32, U64, P]),
        "fa_noise_host": (I, [U64, U32, U32, U64, S, P]),
        "fa_mx8_scale_bytes": (S, [S]),
        "fa_mx8_encode": (I, [P, S, P, P]),
        "fa_mx8_decode": (I, [P, P, S, U64, P]),
        "fa_mx8_expand_device": (I, [P, I, P, P, S, U64, P, I, P, I, P]),
        "fa_set_mx8": (I, [P, I, I]),
        "fa_submit_mx8": (I, [P, I, I, P, P, F, I]),
        "fa_mx8_set_reference": (I, [P, I, P]),
        "fa_mx8_encode_device": (I, [P, I, P, I, P, I, S, U64, P, P, P, I, P]),
        "fa_set_mx8_reply": (I, [P, I, I]),
        "fa_finalize_mx8": (I, [P, I, P, P, I]),
        "fa_copy_mx8": (I, [P, I, P, P, I]),
        "fa_mx8_reply_stats": (I, [P, I, P]),
        "fa_submit": (I, [P, I, I, P, F]),
        "fa_submit_pinned": (I, [P, I, I, P, F]),
        "fa_submit_gather": (I, [P, I, I, I, P, P, F]),
        "fa_submit_gather_pinned": (I, [P, I, I, I, P, P, F]),
        "fa_submit_piece_pinned": (I, [P, I, I, S, P, S]),
        "fa_submit_commit": (I, [P, I, I, F]),
        "fa_finalize": (I, [P, I, P]),
        "fa_finalize_gather": (I, [P, I, I, P, P, I]),
        "fa_host_alloc": (I, [S, ctypes.POINTER(P)]),
        "fa_host_free": (I, [P]),
        "fa_sync_device": (I, [P, I, P, P, I, S, I, P]),
        "fa_sync_part": (I, [P, I, P, P]),
        "fa_bucket_progress": (I, [P, I, ctypes.POINTER(I), ctypes.POINTER(I)]),
        "fa_bucket_host_read": (I, [P, I, ctypes.POINTER(I)]),
        "fa_output_crc32": (I, [P, I, I, ctypes.POINTER(S), ctypes.POINTER(U32)]),
        "fa_reduce_parts": (I, [P, I, ctypes.POINTER(I), P, P]),
        "fa_ctx_set_tuning": (I, [P, ctypes.POINTER(_Tuning)]),
        "fa_ctx_get_tuning": (I, [P, ctypes.POINTER(_Tuning)]),
        "fa_rs_segments": (I, [S, I, I, I, ctypes.POINTER(S), I]),
        "fa_phased_timeouts": (I, [I, ctypes.POINTER(U64)]),
        "fa_release_stream": (I, [I, P]),
        "fa_reduce_device": (I, [P, I, P, P, I, S, I, P, I, I, P, P]),
        "fa_fill_uniform": (I, [P, S, I, U64, U32, U64, P]),
        "fa_diag_read_stream": (I, [P, I, S, P]),  # diagnostics (outside fa.h)
        "fa_diag_read_plain": (I, [P, I, S, I, I, P]),
        "fa_diag_rw_plain": (I, [P, I, S, I, I, I, P]),
        "fa_diag_plan_chain": (I, [I, I, S, I, I, I, ctypes.POINTER(I), ctypes.POINTER(ctypes.c_longlong)]),
        "fa_diag_rs_plan": (I, [S, I, I, I, I, I, I, ctypes.POINTER(I), ctypes.POINTER(I),
                                ctypes.POINTER(ctypes.c_longlong)]),
        "fa_diag_pieces": (I, [S, I, I, ctypes.POINTER(I), ctypes.POINTER(S)]),
        "fa_diag_phased_slot": (I, [I, P, ctypes.POINTER(I)]),
        "fa_diag_phased_owned": (I, [I]),
        "fa_diag_host_reads": (ctypes.c_longlong, [P]),
        "fa_diag_exchange_streams": (I, [P]),
        "fa_set_tuning": (I, [ctypes.POINTER(_Tuning)]),
        "fa_get_tuning": (I, [ctypes.POINTER(_Tuning)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise FaError(rc, lib().fa_last_error().decode(errors="replace"))
    return rc


def last_error():
    return lib().fa_last_error().decode(errors="replace")


def device_count():
    n = ctypes.c_int(0)
    check(lib().fa_device_count(ctypes.byref(n)))
    return n.value


def _addr(x):
    """Device/host address of a torch tensor, numpy array or raw int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    raise TypeError("need a tensor, array or int address, got %r" % type(x))


# Caller streams handed to the library as torch stream objects: (device, hipStream_t) -> live Python objects
# wrapping it.  When the last one is collected the stream is retired and its phased counter slot goes back
# (fa_release_stream); torch's pooled streams are wrapped again later, and simply take a slot anew.  Torch
# stream objects take no weak references, so the tracker rides in the object's __dict__ and goes with it.
_tracked = {}
_tracked_mu = threading.Lock()


class _StreamSlot:
    __slots__ = ("key",)

    def __init__(self, key):
        self.key = key
        with _tracked_mu:
            _tracked[key] = _tracked.get(key, 0) + 1

    def __del__(self):
        try:
            key = self.key
            with _tracked_mu:
                _tracked[key] -= 1
                if _tracked[key]:
                    return
                del _tracked[key]
            if _lib is not None:
                _lib.fa_release_stream(key[0], key[1])
        except Exception:  # interpreter shutdown: module globals may be gone
            pass


def _stream(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    h = stream.cuda_stream  # torch.cuda.Stream on ROCm wraps a hipStream_t
    if h and getattr(stream, "_fa_slot", None) is None:
        dev = stream.device.index if getattr(stream, "device", None) is not None else 0
        try:
            stream._fa_slot = _StreamSlot((dev or 0, h))
        except AttributeError:  # an object without a __dict__: release_stream() by hand
            pass
    return h


def release_stream(stream, device=None):
    """fa_release_stream: give back the phased kernel's owned counter slot of a caller stream (a torch stream
    object or a raw hipStream_t address) before destroying it.  Torch stream objects passed to this module
    are released by themselves when collected; raw handles need this call."""
    if device is None:
        device = stream.device.index if hasattr(stream, "device") and stream.device.index is not None else 0
    h = stream if isinstance(stream, int) else stream.cuda_stream
    check(lib().fa_release_stream(device, h))


def reduce_device(clients, weights, n, in_dtype, out, out_dtype=F32, mode=FEDAVG, init=None, stream=None, gpu=0,
                  ctx=None):
    """fa_reduce_device: D device-resident client buckets -> out (enqueued, not synchronized)."""
    D = len(clients)
    arr = (ctypes.c_void_p * D)(*[_addr(c) for c in clients])
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if w.size != D:
        raise ValueError("need one weight per client")
    check(lib().fa_reduce_device(ctx.handle if ctx is not None else None, gpu, arr, w.ctypes.data, D, n, in_dtype,
                                 _addr(out), out_dtype, mode, _addr(init), _stream(stream)))


def trimmed_device(clients, n, in_dtype, out, out_dtype=F32, trim=TRIM_MEDIAN, stream=None, gpu=0, ctx=None):
    """fa_trimmed_device: the coordinate-wise trimmed mean (trim=TRIM_MEDIAN: the median) of D device-resident
    client buckets -> out (enqueued, not synchronized).  With n == 0 no device is touched: the feature probe."""
    D = len(clients)
    arr = (ctypes.c_void_p * D)(*[_addr(c) for c in clients])
    check(lib().fa_trimmed_device(ctx.handle if ctx is not None else None, gpu, arr, D, n, in_dtype, _addr(out),
                                  out_dtype, trim, _stream(stream)))


def server_opt_device(avg, x, m, v, n, out, out_dtype=F32, rule=OPT_ADAM, lr=1.0, beta1=0.9, beta2=0.99, tau=1e-3,
                      stream=None, gpu=0, ctx=None):
    """fa_server_opt_device: one server-optimizer step on device-resident fp32 arrays -- the aggregate `avg` and
    the state x, m, v (v=None for OPT_MOMENTUM) -- writing the state in place and x' to `out` in out_dtype
    (None: states only; `avg` itself for F32).  Enqueued, not synchronized.  With n == 0 no device is touched:
    the feature probe."""
    opt = _ServerOpt(rule, lr, beta1, beta2, tau)
    check(lib().fa_server_opt_device(ctx.handle if ctx is not None else None, gpu, ctypes.byref(opt), _addr(avg),
                                     _addr(x), _addr(m), _addr(v), n, _addr(out), out_dtype, _stream(stream)))


def clip_sumsq_device(clients, n, in_dtype, ref, stream=None, gpu=0, ctx=None):
    """fa_clip_sumsq_device: the squared L2 distances Q_k (np.float64, one per client) of D device-resident client
    buckets to the fp32 device reference `ref` (fa.h "Clip stage", rule 1).  Enqueued on `stream` and waited for.
    With n == 0 no device is touched and the sums are zeros: the feature probe."""
    D = len(clients)
    arr = (ctypes.c_void_p * D)(*[_addr(c) for c in clients])
    q = np.empty(D, np.float64)
    check(lib().fa_clip_sumsq_device(ctx.handle if ctx is not None else None, gpu, arr, D, n, in_dtype, _addr(ref),
                                     q.ctypes.data, _stream(stream)))
    return q


def clip_scale(sumsq, max_norm):
    """fa_clip_scale (host arithmetic, rule 2): (scale as np.float32, excluded) of a client whose squared
    distance is `sumsq` under the bound `max_norm`; an excluded client (NaN or infinite norm) has scale 0."""
    ex = ctypes.c_int(0)
    s = lib().fa_clip_scale(float(sumsq), float(max_norm), ctypes.byref(ex))
    return np.float32(s), bool(ex.value)


def pairdist_device(clients, n, in_dtype, stream=None, gpu=0, ctx=None):
    """fa_pairdist_device: the pairwise squared L2 distances Q_ab (np.float64, shape (D, D), bit-symmetric, +0
    diagonal) of D device-resident client buckets (fa.h "Krum stage", rule 1).  Enqueued on `stream` and waited
    for.  With n == 0 no device is touched and the matrix is zeros: the feature probe."""
    D = len(clients)
    arr = (ctypes.c_void_p * max(1, D))(*[_addr(c) for c in clients])
    q = np.empty((D, D), np.float64)
    check(lib().fa_pairdist_device(ctx.handle if ctx is not None else None, gpu, arr, D, n, in_dtype, q.ctypes.data,
                                   _stream(stream)))
    return q


def krum_select(dist, f, m=None):
    """fa_krum_select (host arithmetic, rules 2-3): (scores float64[D], selected bool[D]) of the (D, D) matrix
    `dist` with f owners assumed Byzantine and m kept (None: D - f)."""
    dist = np.ascontiguousarray(dist, np.float64)
    D = dist.shape[0] if dist.ndim == 2 else 0
    if dist.ndim != 2 or dist.shape[1] != D:
        raise ValueError("need a square matrix")
    scores, sel = np.empty(D, np.float64), np.empty(D, np.intc)
    ns = ctypes.c_int()
    check(lib().fa_krum_select(dist.ctypes.data, D, int(f), -1 if m is None else int(m), scores.ctypes.data,
                               sel.ctypes.data, ctypes.byref(ns)))
    return scores, sel.astype(bool)


def krum_weights(weights, selected):
    """fa_krum_weights (host arithmetic, rule 4): the weights w' (np.float32, one per client) of a round whose
    selection is `selected`."""
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    sel = np.ascontiguousarray(np.asarray(selected).reshape(-1).astype(np.intc))
    if sel.size != w.size:
        raise ValueError("need one flag per weight")
    out = np.empty(w.size, np.float32)
    check(lib().fa_krum_weights(w.ctypes.data, sel.ctypes.data, w.size, out.ctypes.data))
    return out


def geomed_pass_device(clients, weights, n, in_dtype, v=None, stream=None, gpu=0, ctx=None):
    """fa_geomed_pass_device: one fused Weiszfeld pass over D device-resident client buckets (fa.h "Geomed stage",
    rule 1): (sumsq float64[D], nonfinite float64[D]) -- Q_k against the FEDAVG chain of all D clients under
    `weights`, and the count of NaN / inf elements per bucket; `v` (a device fp32 buffer of n, or None) receives the
    chain.  Enqueued on `stream` and waited for.  With n == 0 no device is touched and both are zeros: the probe."""
    D = len(clients)
    arr = (ctypes.c_void_p * max(1, D))(*[_addr(c) for c in clients])
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if w.size != D:
        raise ValueError("need one weight per client")
    q, b = np.empty(D, np.float64), np.empty(D, np.float64)
    check(lib().fa_geomed_pass_device(ctx.handle if ctx is not None else None, gpu, arr, w.ctypes.data, D, n, in_dtype,
                                      _addr(v), q.ctypes.data, b.ctypes.data, _stream(stream)))
    return q, b


def geomed_weights(weights, sumsq, included, nu=1e-6):
    """fa_geomed_weights (host arithmetic, rules 3-4): (alpha float32[D], included bool[D]) -- the next pass's
    weights from the round's weights, the squared distances Q_k and the clients included so far; a client whose
    distance is NaN or infinite, or whose weight is not > 0, leaves `included` and gets weight 0."""
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    q = np.ascontiguousarray(np.asarray(sumsq, np.float64).reshape(-1))
    inc = np.ascontiguousarray(np.asarray(included).reshape(-1).astype(np.intc))
    if q.size != w.size or inc.size != w.size:
        raise ValueError("need one distance and one flag per weight")
    out = np.empty(w.size, np.float32)
    check(lib().fa_geomed_weights(w.ctypes.data, q.ctypes.data, inc.ctypes.data, w.size, float(nu), out.ctypes.data))
    return out, inc.astype(bool)


def centered_device(clients, n, in_dtype, out, out_dtype=F32, keep=1, stream=None, gpu=0, ctx=None):
    """fa_centered_device: per element the mean of the `keep` values closest to the median of D device-resident
    client buckets -> out (fa.h "Bulyan stage", rule 4; enqueued, not synchronized).  With n == 0 no device is
    touched: the feature probe."""
    D = len(clients)
    arr = (ctypes.c_void_p * max(1, D))(*[_addr(c) for c in clients])
    check(lib().fa_centered_device(ctx.handle if ctx is not None else None, gpu, arr, D, n, in_dtype, _addr(out),
                                   out_dtype, int(keep), _stream(stream)))


def bulyan_select(dist, f):
    """fa_bulyan_select (host arithmetic, rule 2): (order, pick_scores, selected bool[D]) of the (D, D) matrix
    `dist` with f owners assumed Byzantine: the picks in pick order (np.intc) and the score each was picked with
    (np.float64), both as long as the number picked."""
    dist = np.ascontiguousarray(dist, np.float64)
    D = dist.shape[0] if dist.ndim == 2 else 0
    if dist.ndim != 2 or dist.shape[1] != D:
        raise ValueError("need a square matrix")
    order, ps, sel = np.empty(D, np.intc), np.empty(D, np.float64), np.empty(D, np.intc)
    ns = ctypes.c_int()
    check(lib().fa_bulyan_select(dist.ctypes.data, D, int(f), order.ctypes.data, ps.ctypes.data, sel.ctypes.data,
                                 ctypes.byref(ns)))
    return order[:ns.value].copy(), ps[:ns.value].copy(), sel.astype(bool)


def noise_device(avg, n, out, out_dtype=F32, stddev=1.0, seed=0, stream_id=0, round=0, idx0=0, stream=None, gpu=0,
                 ctx=None):
    """fa_noise_device: out[i] = avg[i] + stddev z_{idx0 + i} over n device-resident fp32 (fa.h "Noise stage"), out in
    out_dtype with one rounding (`avg` itself for F32: in place).  stream_id is the generator's stream word (the
    library uses the part id), `stream` the HIP stream.  Enqueued, not synchronized.  With n == 0 no device is
    touched: the feature probe."""
    check(lib().fa_noise_device(ctx.handle if ctx is not None else None, gpu, _addr(avg), n, _addr(out), out_dtype,
                                float(stddev), int(seed), int(stream_id), int(round), int(idx0), _stream(stream)))


def noise_host(seed, stream_id, round, idx0, n):
    """fa_noise_host (host arithmetic): the n unit normals (np.float32) of bucket elements idx0 .. idx0 + n - 1 under
    (seed, stream_id, round), the bits the kernel adds."""
    z = np.empty(n, np.float32)
    check(lib().fa_noise_host(int(seed), int(stream_id), int(round), int(idx0), n, z.ctypes.data))
    return z


MX8_BLOCK = 32  # FA_MX8_BLOCK: elements per scale byte of an MX8 receipt (fa.h "MX8 receipts")
MX8_ABSOLUTE = 0x2  # FA_MX8_ABSOLUTE
MX8_SCALES_ONLY, MX8_SCALES_GIVEN = 0x1, 0x2  # FA_MX8_SCALES_ONLY, FA_MX8_SCALES_GIVEN (mx8_encode_device)


def mx8_scale_bytes(n):
    """fa_mx8_scale_bytes: ceil(n / 32)."""
    return lib().fa_mx8_scale_bytes(n)


def mx8_encode(delta):
    """fa_mx8_encode (host arithmetic, the owner's side): the fp32 deltas as (q int8[n], e uint8[ceil(n / 32)])."""
    delta = np.ascontiguousarray(np.asarray(delta, np.float32).reshape(-1))
    q, e = np.empty(delta.size, np.int8), np.empty(mx8_scale_bytes(delta.size), np.uint8)
    check(lib().fa_mx8_encode(delta.ctypes.data, delta.size, q.ctypes.data, e.ctypes.data))
    return q, e


def mx8_decode(q, e, idx0=0):
    """fa_mx8_decode (host arithmetic): the fp32 deltas of bucket elements idx0 .. idx0 + len(q) - 1; e[0] is the
    scale of block idx0 >> 5."""
    q = np.ascontiguousarray(np.asarray(q, np.int8).reshape(-1))
    e = np.ascontiguousarray(np.asarray(e, np.uint8).reshape(-1))
    if q.size and e.size < ((idx0 + q.size - 1) >> 5) - (idx0 >> 5) + 1:
        raise ValueError("e holds %d scales, elements [%d, %d) touch more blocks" % (e.size, idx0, idx0 + q.size))
    d = np.empty(q.size, np.float32)
    check(lib().fa_mx8_decode(q.ctypes.data, e.ctypes.data, q.size, int(idx0), d.ctypes.data))
    return d


def mx8_expand_device(q, e, n, dst, dst_dtype=F32, ref=None, ref_dtype=F32, idx0=0, stream=None, gpu=0, ctx=None):
    """fa_mx8_expand_device: dst[i] = ref[i] + d_i over n device-resident elements (ref None: absolute mode, dst[i] =
    d_i), q / e / idx0 as for mx8_decode, device pointers of any byte (q, e) or element (ref, dst) phase.  Enqueued,
    not synchronized.  With n == 0 no device is touched: the feature probe."""
    check(lib().fa_mx8_expand_device(ctx.handle if ctx is not None else None, gpu, _addr(q), _addr(e), n, int(idx0),
                                     _addr(ref), ref_dtype, _addr(dst), dst_dtype, _stream(stream)))


def mx8_encode_device(new, sent, n, q, e, out=None, dtype=F32, sent_dtype=None, idx0=0, scales_only=False,
                      scales_given=False, stream=None, gpu=0, ctx=None):
    """fa_mx8_encode_device (fa.h "MX8 replies", rules 3-4): over n device-resident elements of `dtype`, bucket elements
    idx0 .., the codes q and the scales e of fl(new - sent), and (out not None) g' = sent + decode(q, e) into out, which
    may be `sent` or `new` itself.  scales_only: e alone is written; scales_given: e is read.  Enqueued, not
    synchronized.  With n == 0 no device is touched: the feature probe."""
    flags = (MX8_SCALES_ONLY if scales_only else 0) | (MX8_SCALES_GIVEN if scales_given else 0)
    check(lib().fa_mx8_encode_device(ctx.handle if ctx is not None else None, gpu, _addr(new), dtype, _addr(sent),
                                     dtype if sent_dtype is None else sent_dtype, n, int(idx0), _addr(q), _addr(e),
                                     _addr(out), flags, _stream(stream)))


def sync_device(clients, weights, n, dtype, stream=None, gpu=0, ctx=None):
    """fa_sync_device: every device bucket in `clients` := sum_k w_k clients[k] (in place, enqueued)."""
    D = len(clients)
    arr = (ctypes.c_void_p * D)(*[_addr(c) for c in clients])
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if w.size != D:
        raise ValueError("need one weight per client")
    check(lib().fa_sync_device(ctx.handle if ctx is not None else None, gpu, arr, w.ctypes.data, D, n, dtype,
                               _stream(stream)))


def fill_uniform(dst, n, dtype, seed, client, idx0=0, stream=None):
    check(lib().fa_fill_uniform(_addr(dst), n, dtype, seed, client, idx0, _stream(stream)))


def diag_read_stream(buffers, n, stream=None):
    """fa_diag_read_stream (diagnostic, outside fa.h): one read-only launch over the fp32 device buffers
    (n elements each, n % 4 == 0, 16-byte aligned) on `stream`; time it with events on that stream."""
    arr = (ctypes.c_void_p * len(buffers))(*[_addr(b) for b in buffers])
    check(lib().fa_diag_read_stream(arr, len(buffers), n, _stream(stream)))


def diag_read_plain(buffers, n, grid=8192, unroll=16, stream=None):
    """fa_diag_read_plain (diagnostic, outside fa.h): the independent read ceiling -- one plain grid-stride
    launch (`grid` workgroups of 256 lanes, `unroll` nt 16-byte loads in flight) reading the fp32 device
    buffers (n elements each) one after another, on `stream`."""
    arr = (ctypes.c_void_p * len(buffers))(*[_addr(b) for b in buffers])
    check(lib().fa_diag_read_plain(arr, len(buffers), n, grid, unroll, _stream(stream)))


def diag_rw_plain(buffers, n, grid=8192, unroll=16, nt=False, stream=None):
    """fa_diag_rw_plain (diagnostic, outside fa.h): the independent in-place read+write ceiling -- one plain
    grid-stride launch reading every fp32 device buffer (n elements each) and writing it back where it lies
    (values unchanged), buffer after buffer, nt loads and plain (or nt) stores, on `stream`."""
    arr = (ctypes.c_void_p * len(buffers))(*[_addr(b) for b in buffers])
    check(lib().fa_diag_rw_plain(arr, len(buffers), n, grid, unroll, 1 if nt else 0, _stream(stream)))


PLAN_ONE_SHOT, PLAN_SCALAR, PLAN_PHASED = 0, 1, 2


def plan_chain(in_dtype, out_dtype, n, n_clients, walk=0, cus=256):
    """fa_diag_plan_chain (diagnostic, host arithmetic): (kind, phases) of the launch one FedAvg chain over a
    16-byte aligned bucket of n elements takes under fa_tuning.walk `walk` (0 = the process default) on `cus`
    CUs; kind PLAN_PHASED with phases > 1 means chip-wide meetings.  F16 takes the plans of BF16; a
    BF16 <-> F16 pair raises FaError(ERR_ARG)."""
    k, ph = ctypes.c_int(), ctypes.c_longlong()
    check(lib().fa_diag_plan_chain(in_dtype, out_dtype, n, n_clients, walk, cus, ctypes.byref(k), ctypes.byref(ph)))
    return k.value, ph.value


def rs_plan(n, n_gpus, n_clients, chunks=0, in_dtype=F32, out_dtype=F32, cus=256):
    """fa_diag_rs_plan (diagnostic): (launches, phased launches, most phases of one launch) that one
    FA_SHARD_CLIENT_RS round enqueues for a bucket of n elements (the process-default tuning)."""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    check(lib().fa_diag_rs_plan(n, n_gpus, n_clients, chunks, in_dtype, out_dtype, cus, ctypes.byref(a),
                                ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def piece_plan(n, held, in_dtype=F32):
    """fa_diag_pieces (diagnostic): (pieces, elements per piece) of a range-layout GPU holding `held` slots of
    n elements (under the process-default piece_span_kib / piece_split_kib, set_tuning)."""
    a, b = ctypes.c_int(), ctypes.c_size_t()
    check(lib().fa_diag_pieces(n, held, in_dtype, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def _tuning_dict(t):
    return {"block": t.block, "max_blocks": t.max_blocks, "unroll": t.unroll, "load_policy": t.load_policy,
            "store_policy": t.store_policy, "slot_skew": t.slot_skew, "walk": t.walk, "rs_chunks": t.rs_chunks,
            "piece_span_kib": t.piece_span_kib, "piece_split_kib": t.piece_split_kib}


def get_tuning():
    """fa_get_tuning: the process defaults (new contexts and context-less calls start from them)."""
    t = _Tuning()
    check(lib().fa_get_tuning(ctypes.byref(t)))
    return _tuning_dict(t)


LOAD_DEFAULT, LOAD_NT = 1, 2
STORE_PLAIN, STORE_NT, STORE_SC1, STORE_SC01 = 1, 2, 3, 4


def set_tuning(block=0, max_blocks=0, unroll=0, load_policy=0, store_policy=0, slot_skew=0, walk=0, rs_chunks=0,
               piece_span_kib=0, piece_split_kib=0):
    """fa_set_tuning (process defaults); every argument 0 = keep.  max_blocks -1 = one-shot grid,
    slot_skew -1 = none, -2 = by slot size (the default: 512 B from 48 MiB slots up, else 2048);
    piece_span_kib -1 = never cut a GPU's slots into range pieces, piece_split_kib -1 = always cut them."""
    t = _Tuning(block, max_blocks, unroll, load_policy, store_policy, slot_skew, walk, rs_chunks, piece_span_kib,
                piece_split_kib)
    check(lib().fa_set_tuning(ctypes.byref(t)))


def phased_timeouts(device=0):
    """fa_phased_timeouts: phased-kernel meetings on `device` whose bounded wait ran out (grid not
    co-resident) since the process started."""
    c = ctypes.c_uint64()
    check(lib().fa_phased_timeouts(device, ctypes.byref(c)))
    return c.value


def phased_slot(stream, device=0):
    """fa_diag_phased_slot (diagnostic): (counter slot, owned) of the phased kernel for `stream` on `device`,
    assigned now if the stream has none yet -- owned: the slot is the stream's alone (the first 48 streams,
    until their context is destroyed), else a hashed slot shared with other streams."""
    own = ctypes.c_int()
    slot = lib().fa_diag_phased_slot(device, _stream(stream), ctypes.byref(own))
    if slot < 0:
        check(slot)
    return slot, bool(own.value)


def phased_owned_slots(device=0):
    """fa_diag_phased_owned (diagnostic): how many of the 48 owned counter slots are taken on `device`."""
    n = lib().fa_diag_phased_owned(device)
    if n < 0:
        check(n)
    return n


def rs_segments(n, n_gpus, chunks, gpu):
    """fa_rs_segments: [(lo, hi), ...] of bucket elements GPU `gpu` holds after the rs layout's
    reduce-scatter (block-cyclic over `chunks` pieces), in the order of its shard."""
    cnt = lib().fa_rs_segments(n, n_gpus, chunks, gpu, None, 0)
    if cnt < 0:
        check(cnt)
    buf = (ctypes.c_size_t * (2 * max(1, cnt)))()
    lib().fa_rs_segments(n, n_gpus, chunks, gpu, buf, cnt)
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(cnt)]


HOST_PINNED = 0x1


class PinnedBuffer:
    """fa_host_alloc'd page-locked host memory, viewed as a numpy array (freed on close / GC)."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        check(lib().fa_host_alloc(nbytes, ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes

    def view(self, dtype=np.uint8, count=-1, offset=0):
        if not self.ptr:
            return np.empty(0, dtype)
        raw = (ctypes.c_char * self.nbytes).from_address(self.ptr)
        return np.frombuffer(raw, dtype=dtype, count=count, offset=offset)

    def close(self):
        if self.ptr:
            check(lib().fa_host_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _segments(pieces):
    pieces = [np.ascontiguousarray(x) for x in pieces]
    ptrs = (ctypes.c_void_p * len(pieces))(*[x.ctypes.data for x in pieces])
    sizes = (ctypes.c_size_t * len(pieces))(*[x.nbytes for x in pieces])
    return pieces, ptrs, sizes


class Aggregator:
    """fa_ctx: the aggregator's global parts on 1..G GPUs (range-sharded when G > 1).

    Usage mirrors one aggregation phase of aggregator.cpp: define the bucket
    once (refactor), submit every receipt, finalize to obtain the reduced part.
    """

    def __init__(self, n_gpus=1, flags=None, devices=None, rs=False, eager=False, shared_device=False):
        if devices is None:
            devices = list(range(n_gpus))
        n_gpus = len(devices)
        if flags is None:
            flags = SHARD_CLIENT_RS if rs else SHARD_RANGE if n_gpus > 1 else 0
            flags |= (ACCUMULATE_ON_ARRIVAL if eager else 0) | (TEST_SHARED_DEVICE if shared_device else 0)
        h = ctypes.c_void_p()
        ids = (ctypes.c_int * n_gpus)(*devices)
        check(lib().fa_create_ex(ctypes.byref(h), ids, n_gpus, flags))
        self.devices = list(devices)
        self.handle = h
        self.parts = {}

    def define(self, part_id, n, in_dtype=F32, out_dtype=F32, n_clients=1, mode=FEDAVG, trim=None):
        check(lib().fa_bucket_define(self.handle, part_id, n, in_dtype, out_dtype, n_clients, mode))
        self.parts[part_id] = (n, in_dtype, out_dtype, n_clients, mode)
        if trim is not None:
            self.set_trim(trim, part_id)

    def set_divisor(self, divisor, part_id=-1):
        check(lib().fa_set_literal_divisor(self.handle, part_id, divisor))

    def set_trim(self, trim, part_id=-1):
        """fa_set_trim: the trim of a TRIMMED part (part_id < 0: the default of parts defined later)."""
        check(lib().fa_set_trim(self.handle, part_id, trim))

    def set_server_opt(self, rule, lr=0.0, beta1=0.9, beta2=0.99, tau=1e-3, part_id=-1):
        """fa_set_server_opt: the server-optimizer stage of a part (part_id < 0: the default of FEDAVG and
        TRIMMED parts defined later).  The same rule again changes only the hyperparameters; another rule
        keeps x and zeroes m and v; OPT_NONE removes the stage."""
        opt = _ServerOpt(rule, lr, beta1, beta2, tau)
        check(lib().fa_set_server_opt(self.handle, part_id, ctypes.byref(opt)))

    def server_opt(self, part_id=-1):
        """fa_get_server_opt: (rule, lr, beta1, beta2, tau) of the part's stage (rule OPT_NONE: none), or of
        the context default (part_id < 0)."""
        opt = _ServerOpt()
        check(lib().fa_get_server_opt(self.handle, part_id, ctypes.byref(opt)))
        return opt.rule, opt.lr, opt.beta1, opt.beta2, opt.tau

    def server_opt_state(self, part_id):
        """fa_server_opt_get_state: (x, m, v, steps) of the part's stage as whole-bucket fp32 numpy arrays
        (v is None for OPT_MOMENTUM, which has none)."""
        n = self.parts[part_id][0]
        x, m = np.empty(n, np.float32), np.empty(n, np.float32)
        v = None if self.server_opt(part_id)[0] == OPT_MOMENTUM else np.empty(n, np.float32)
        steps = ctypes.c_uint64()
        check(lib().fa_server_opt_get_state(self.handle, part_id, x.ctypes.data, m.ctypes.data,
                                            None if v is None else v.ctypes.data, ctypes.byref(steps)))
        return x, m, v, steps.value

    def set_server_opt_state(self, part_id, x=None, m=None, v=None, steps=None):
        """fa_server_opt_set_state: scatter whole-bucket fp32 arrays into the stage's state (None: leave that
        array as it is); with an x the part has a master, so its next reduction is a step, not the bootstrap.
        steps=None keeps the count."""
        n = self.parts[part_id][0]
        arrs = []
        for a in (x, m, v):
            if a is not None:
                a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
                if a.size != n:
                    raise ValueError("bucket %d holds %d elements, got %d" % (part_id, n, a.size))
            arrs.append(a)
        if steps is None:
            cur = ctypes.c_uint64()
            check(lib().fa_server_opt_get_state(self.handle, part_id, None, None, None, ctypes.byref(cur)))
            steps = cur.value
        check(lib().fa_server_opt_set_state(self.handle, part_id, *[None if a is None else a.ctypes.data for a in arrs],
                                            int(steps)))

    def set_clip(self, max_norm, part_id=-1):
        """fa_set_clip: per-client L2 norm clipping of a FEDAVG part's updates to `max_norm` (part_id < 0: the
        default of FEDAVG parts defined later); 0 removes the stage."""
        check(lib().fa_set_clip(self.handle, part_id, float(max_norm)))

    def clip_round(self, part_id):
        """fa_clip_get_round: (sumsq float64[D], scales float32[D], included bool[D], n_clipped) of the part's
        last reducing call; an excluded client has scale 0."""
        D = self.parts[part_id][3]
        q, s, inc = np.empty(D, np.float64), np.empty(D, np.float32), np.empty(D, np.intc)
        nc = ctypes.c_int()
        check(lib().fa_clip_get_round(self.handle, part_id, q.ctypes.data, s.ctypes.data, inc.ctypes.data,
                                      ctypes.byref(nc)))
        return q, s, inc.astype(bool), nc.value

    def clip_reference(self, part_id):
        """fa_clip_get_reference: the part's reference g as a whole-bucket fp32 numpy array."""
        g = np.empty(self.parts[part_id][0], np.float32)
        check(lib().fa_clip_get_reference(self.handle, part_id, g.ctypes.data))
        return g

    def set_clip_reference(self, part_id, g):
        """fa_clip_set_reference: scatter a whole-bucket fp32 array into the part's reference; None drops the
        reference, so the next round bootstraps."""
        if g is not None:
            g = np.ascontiguousarray(np.asarray(g, np.float32).reshape(-1))
            if g.size != self.parts[part_id][0]:
                raise ValueError("bucket %d holds %d elements, got %d" % (part_id, self.parts[part_id][0], g.size))
        check(lib().fa_clip_set_reference(self.handle, part_id, None if g is None else g.ctypes.data))

    def set_krum(self, f, m=None, part_id=-1):
        """fa_set_krum: Krum / Multi-Krum selection on a FEDAVG part with f owners assumed Byzantine and m kept
        (None: D - f; 1: Krum; part_id < 0: the default of FEDAVG parts defined later); m=0 removes the stage."""
        check(lib().fa_set_krum(self.handle, part_id, int(f), -1 if m is None else int(m)))

    def krum_round(self, part_id):
        """fa_krum_get_round: (dist float64[D, D], scores float64[D], selected bool[D]) of the part's last
        reducing call."""
        D = self.parts[part_id][3]
        q, s, sel = np.empty((D, D), np.float64), np.empty(D, np.float64), np.empty(D, np.intc)
        ns = ctypes.c_int()
        check(lib().fa_krum_get_round(self.handle, part_id, q.ctypes.data, s.ctypes.data, sel.ctypes.data,
                                      ctypes.byref(ns)))
        return q, s, sel.astype(bool)

    def set_geomed(self, iters, nu=1e-6, part=None):
        """fa_set_geomed: the geometric median (RFA: `iters` smoothed Weiszfeld passes with the distance floor `nu`)
        on a FEDAVG part (part=None: the default of FEDAVG parts defined later); iters=0 removes the stage."""
        check(lib().fa_set_geomed(self.handle, -1 if part is None else part, int(iters), float(nu)))

    def geomed(self, part=None):
        """fa_get_geomed: (iters, nu) of the part's stage (iters 0: none), or of the context default."""
        it, nu = ctypes.c_int(), ctypes.c_float()
        check(lib().fa_get_geomed(self.handle, -1 if part is None else part, ctypes.byref(it), ctypes.byref(nu)))
        return it.value, nu.value

    def geomed_round(self, part):
        """fa_geomed_get_round: the trace of the part's last reducing call as (sumsq float64[P, D], weights
        float32[P + 1, D], included bool[D], objective float64[P]) over its P valid passes; the last row of
        `weights` is the final chain's."""
        D = self.parts[part][3]
        q = np.zeros((GEOMED_MAX_ITERS, D), np.float64)
        w = np.zeros((GEOMED_MAX_ITERS + 1, D), np.float32)
        inc, obj = np.empty(D, np.intc), np.zeros(GEOMED_MAX_ITERS, np.float64)
        npass = ctypes.c_int()
        check(lib().fa_geomed_get_round(self.handle, part, ctypes.byref(npass), q.ctypes.data, w.ctypes.data,
                                        inc.ctypes.data, obj.ctypes.data))
        t = npass.value
        return q[:t].copy(), w[:t + 1].copy(), inc.astype(bool), obj[:t].copy()

    def set_bulyan(self, f, part_id=-1):
        """fa_set_bulyan: the Bulyan stage (iterated Krum, then a median-centred mean) on a TRIMMED part with f
        owners assumed Byzantine (part_id < 0: the default of TRIMMED parts defined later); f=None removes it."""
        check(lib().fa_set_bulyan(self.handle, part_id, -1 if f is None else int(f)))

    def bulyan_round(self, part_id):
        """fa_bulyan_get_round: (dist float64[D, D], order, pick_scores, selected bool[D]) of the part's last
        reducing call; order and pick_scores are as long as the number picked, in pick order."""
        D = self.parts[part_id][3]
        q, order, ps, sel = (np.empty((D, D), np.float64), np.empty(D, np.intc), np.empty(D, np.float64),
                             np.empty(D, np.intc))
        ns = ctypes.c_int()
        check(lib().fa_bulyan_get_round(self.handle, part_id, q.ctypes.data, order.ctypes.data, ps.ctypes.data,
                                        sel.ctypes.data, ctypes.byref(ns)))
        return q, order[:ns.value].copy(), ps[:ns.value].copy(), sel.astype(bool)

    def set_noise(self, stddev, seed, part_id=-1):
        """fa_set_noise: Gaussian noise of standard deviation `stddev` on the part's fp32 aggregate, drawn from
        `seed` (u64), the part id and the part's round counter (part_id < 0: the default of FEDAVG and TRIMMED parts
        defined later); again changes stddev and seed and keeps the round; stddev=0 removes the stage."""
        check(lib().fa_set_noise(self.handle, part_id, float(stddev), int(seed)))

    def noise(self, part_id=-1):
        """fa_get_noise: (stddev, seed) of the part's stage (stddev 0: none), or of the context default."""
        sd, seed = ctypes.c_float(), ctypes.c_uint64()
        check(lib().fa_get_noise(self.handle, part_id, ctypes.byref(sd), ctypes.byref(seed)))
        return sd.value, seed.value

    def noise_round(self, part_id):
        """fa_noise_get_round: the round the part's next reducing call draws its noise from."""
        r = ctypes.c_uint64()
        check(lib().fa_noise_get_round(self.handle, part_id, ctypes.byref(r)))
        return r.value

    def set_noise_round(self, part_id, r):
        """fa_noise_set_round: replay a round, or continue a sequence after a restart."""
        check(lib().fa_noise_set_round(self.handle, part_id, int(r)))

    def submit(self, part_id, slot, host, weight=1.0, pinned=False):
        host = np.ascontiguousarray(host)
        if part_id not in self.parts:
            check(lib().fa_submit(self.handle, part_id, slot, host.ctypes.data, float(weight)))
        n, in_dtype = self.parts[part_id][:2]
        if host.nbytes != n * DTYPE_SIZE[in_dtype]:
            raise ValueError("bucket %d expects %d bytes, got %d" % (part_id, n * DTYPE_SIZE[in_dtype], host.nbytes))
        fn = lib().fa_submit_pinned if pinned else lib().fa_submit
        check(fn(self.handle, part_id, slot, host.ctypes.data, float(weight)))

    def set_mx8(self, on=True, part_id=-1):
        """fa_set_mx8: the part takes MX8 receipts and keeps its device output as their reference (part_id < 0: the
        default of parts defined later); on=False frees what it allocated."""
        check(lib().fa_set_mx8(self.handle, part_id, 1 if on else 0))

    def submit_mx8(self, part_id, slot, q, e, weight=1.0, pinned=False, absolute=False):
        """fa_submit_mx8: the client's update against the part's last output as (q int8[n], e uint8[ceil(n / 32)]),
        expanded into the slot on the GPU.  pinned: views of PinnedBuffers the caller keeps unchanged until finalize
        returns.  absolute: the values themselves, no reference."""
        q, e = np.ascontiguousarray(q), np.ascontiguousarray(e)
        if q.dtype != np.int8 or e.dtype != np.uint8:
            raise ValueError("need q int8 and e uint8")
        if part_id in self.parts:
            n = self.parts[part_id][0]
            if q.size != n or e.size != mx8_scale_bytes(n):
                raise ValueError("bucket %d expects %d codes and %d scales, got %d and %d"
                                 % (part_id, n, mx8_scale_bytes(n), q.size, e.size))
        flags = (HOST_PINNED if pinned else 0) | (MX8_ABSOLUTE if absolute else 0)
        check(lib().fa_submit_mx8(self.handle, part_id, slot, q.ctypes.data, e.ctypes.data, float(weight), flags))

    def set_mx8_reference(self, part_id, g):
        """fa_mx8_set_reference: the part's device output := g (n elements of the out dtype; bf16 as uint16 bits), the
        reference of the next relative submits."""
        g = np.ascontiguousarray(g)
        if part_id in self.parts:
            n, _, out_dtype = self.parts[part_id][:3]
            if g.nbytes != n * DTYPE_SIZE[out_dtype]:
                raise ValueError("bucket %d's output holds %d bytes, got %d" % (part_id, n * DTYPE_SIZE[out_dtype], g.nbytes))
        check(lib().fa_mx8_set_reference(self.handle, part_id, g.ctypes.data))

    def set_mx8_reply(self, on=True, part_id=-1):
        """fa_set_mx8_reply: the part's new model goes back as MX8 codes against the model the owners were last sent,
        and its output becomes what they hold after it (part_id < 0: the default of parts defined later); on=False
        frees the sent model and the codes."""
        check(lib().fa_set_mx8_reply(self.handle, part_id, 1 if on else 0))

    def _mx8_codes(self, fn, part_id):
        if part_id not in self.parts:  # let the library report it (FA_ERR_ARG)
            check(fn(self.handle, part_id, None, None, 0))
        n = self.parts[part_id][0]
        q, e = np.empty(n, np.int8), np.empty(mx8_scale_bytes(n), np.uint8)
        check(fn(self.handle, part_id, q.ctypes.data, e.ctypes.data, 0))
        return q, e

    def finalize_mx8(self, part_id):
        """fa_finalize_mx8: ends the round as finalize does and returns its codes (q int8[n], e uint8[ceil(n / 32)])
        instead of the bucket; FA_ERR_STATE, the round untouched, when the owners hold no model yet."""
        return self._mx8_codes(lib().fa_finalize_mx8, part_id)

    def copy_mx8(self, part_id):
        """fa_copy_mx8: the codes (q, e) of the part's last reducing call."""
        return self._mx8_codes(lib().fa_copy_mx8, part_id)

    def mx8_reply_stats(self, part_id):
        """fa_mx8_reply_stats: the E = 255 (NaN) blocks among the codes of the part's last reducing call."""
        nan = ctypes.c_uint64()
        check(lib().fa_mx8_reply_stats(self.handle, part_id, ctypes.byref(nan)))
        return nan.value

    def submit_gather(self, part_id, slot, pieces, weight=1.0, pinned=False):
        """fa_submit_gather(_pinned): `pieces` (host arrays) concatenate to the bucket.  pinned: views of
        PinnedBuffers the caller keeps unchanged until finalize returns."""
        pieces, ptrs, sizes = _segments(pieces)
        fn = lib().fa_submit_gather_pinned if pinned else lib().fa_submit_gather
        check(fn(self.handle, part_id, slot, len(pieces), ptrs, sizes, float(weight)))

    def submit_piece(self, part_id, slot, byte_offset, piece):
        """fa_submit_piece_pinned: bytes [byte_offset, + piece.nbytes) of the slot from `piece`, a view of a
        PinnedBuffer the caller keeps unchanged until finalize returns; submit_commit makes them a receipt."""
        piece = np.ascontiguousarray(piece)
        check(lib().fa_submit_piece_pinned(self.handle, part_id, slot, byte_offset, piece.ctypes.data, piece.nbytes))

    def submit_commit(self, part_id, slot, weight=1.0):
        check(lib().fa_submit_commit(self.handle, part_id, slot, float(weight)))

    def sync_states(self, part_id, weights=None, stream=None):
        """fa_sync_part: every client slot of the part := the FedAvg of all slots (in place, async)."""
        wp = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights, np.float32))
            self._w_keep = w
            wp = w.ctypes.data
        check(lib().fa_sync_part(self.handle, part_id, wp, _stream(stream)))

    def finalize_gather(self, part_id, pieces, pinned=False):
        """fa_finalize_gather: the reduced bucket scattered over `pieces` (writable host arrays)."""
        for x in pieces:
            if not (isinstance(x, np.ndarray) and x.flags.c_contiguous and x.flags.writeable):
                raise ValueError("finalize_gather needs writable contiguous arrays")
        _, ptrs, sizes = _segments(pieces)
        check(lib().fa_finalize_gather(self.handle, part_id, len(pieces), ptrs, sizes, HOST_PINNED if pinned else 0))

    def finalize(self, part_id, out=None):
        if part_id not in self.parts:  # let the library report it (FA_ERR_ARG)
            check(lib().fa_finalize(self.handle, part_id, None))
        n, _, out_dtype = self.parts[part_id][:3]
        if out is None:
            out = np.empty(n, _OUT_NP[out_dtype])
        check(lib().fa_finalize(self.handle, part_id, out.ctypes.data))
        return out

    def slot(self, part_id, gpu, client_slot):
        """(device address, n_elems, elem_offset) of a client slot."""
        ptr, n, off = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().fa_bucket_slot(self.handle, part_id, gpu, client_slot, ctypes.byref(ptr), ctypes.byref(n),
                                   ctypes.byref(off)))
        return ptr.value, n.value, off.value

    def pieces(self, part_id, gpu, client_slot):
        """[(device address, n_elems, elem_offset)] of every piece of a client slot, in element order (one
        entry unless the GPU's slots span more than the piece threshold, fa_bucket_pieces)."""
        npc = ctypes.c_int()
        check(lib().fa_bucket_pieces(self.handle, part_id, gpu, ctypes.byref(npc)))
        out = []
        for j in range(npc.value):
            ptr, n, off = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
            check(lib().fa_bucket_piece(self.handle, part_id, gpu, j, client_slot, ctypes.byref(ptr),
                                        ctypes.byref(n), ctypes.byref(off)))
            out.append((ptr.value, n.value, off.value))
        return out

    def progress(self, part_id):
        """fa_bucket_progress: (receipts submitted this round, leading slots already reduced)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        check(lib().fa_bucket_progress(self.handle, part_id, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def host_read_kept(self, part_id):
        """fa_bucket_host_read: True when the part's round so far is kept host-side to be read in place."""
        k = ctypes.c_int()
        check(lib().fa_bucket_host_read(self.handle, part_id, ctypes.byref(k)))
        return bool(k.value)

    def reduce_parts(self, part_ids, weights=None, stream=None):
        """fa_reduce_parts: one batched reduction of several parts (async); weights: None or one array per
        part (None entries = the submitted weights)."""
        ids = (ctypes.c_int * len(part_ids))(*part_ids)
        wp = None
        if weights is not None:
            keep = [None if w is None else np.ascontiguousarray(np.asarray(w, np.float32)) for w in weights]
            self._w_keep = keep
            wp = (ctypes.c_void_p * len(part_ids))(*[None if w is None else w.ctypes.data for w in keep])
        check(lib().fa_reduce_parts(self.handle, len(part_ids), ids, wp, _stream(stream)))

    def set_tuning(self, **kw):
        """fa_ctx_set_tuning: this context's tuning (same keys as set_tuning; 0 = keep)."""
        t = _Tuning(*[kw.get(k, 0) for k, _ in _Tuning._fields_])
        check(lib().fa_ctx_set_tuning(self.handle, ctypes.byref(t)))

    def get_tuning(self):
        t = _Tuning()
        check(lib().fa_ctx_get_tuning(self.handle, ctypes.byref(t)))
        return _tuning_dict(t)

    def output(self, part_id, gpu=0):
        ptr = ctypes.c_void_p()
        check(lib().fa_bucket_output(self.handle, part_id, gpu, ctypes.byref(ptr)))
        return ptr.value

    def reduce(self, part_id, weights=None, stream=None):
        """fa_reduce_part: device-resident reduction of the part's slots (async)."""
        wp = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights, np.float32))
            self._w_keep = w
            wp = w.ctypes.data
        check(lib().fa_reduce_part(self.handle, part_id, wp, _stream(stream)))

    def copy_output(self, part_id, out=None):
        n, _, out_dtype = self.parts[part_id][:3]
        if out is None:
            out = np.empty(n, _OUT_NP[out_dtype])
        check(lib().fa_copy_output(self.handle, part_id, out.ctypes.data))
        return out

    def output_crc32(self, part_id, seg_bytes):
        """fa_output_crc32: zlib CRC-32 of consecutive byte segments of the part's device output (GPU-side)."""
        n = len(seg_bytes)
        b = (ctypes.c_size_t * max(1, n))(*seg_bytes)
        out = (ctypes.c_uint32 * max(1, n))()
        check(lib().fa_output_crc32(self.handle, part_id, n, b, out))
        return [out[i] for i in range(n)]

    def sync(self):
        check(lib().fa_sync(self.handle))

    def host_reads(self):
        """fa_diag_host_reads (diagnostic): reductions of this context that read their receipts where they
        arrived (small pinned receipts of a one-GPU range part)."""
        return lib().fa_diag_host_reads(self.handle)

    def exchange_streams(self):
        """fa_diag_exchange_streams (diagnostic): GPUs of this context holding an exchange stream (rs only)."""
        return lib().fa_diag_exchange_streams(self.handle)

    def close(self):
        if self.handle:
            lib().fa_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
