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
DNC_MAX_CLIENTS, DNC_MAX_ITERS = 128, 1024  # FA_DNC_MAX_*: the DnC stage, gram_device and dnc_select
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
        "fa_gram_device": (I, [P, I, P, I, S, I, P, P, P]),
        "fa_set_dnc": (I, [P, I, I, I]),
        "fa_dnc_get_round": (I, [P, I, P, P, P, ctypes.POINTER(I)]),
        "fa_dnc_select": (I, [P, I, I, I, P, P, ctypes.POINTER(I)]),
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
        "fa_topk_encode": (I, [P, S, S, P, P, P]),
        "fa_topk_decode": (I, [P, P, S, U64, S, P]),
        "fa_topk_expand_device": (I, [P, I, P, P, S, S, U64, P, I, P, I, P]),
        "fa_topk_encode_workspace": (S, [S]),
        "fa_topk_encode_device": (I, [P, I, P, I, P, I, S, S, P, P, P, P, P]),
        "fa_set_topk": (I, [P, I, S]),
        "fa_submit_topk": (I, [P, I, I, P, P, S, F, I]),
        "fa_lowrank_check": (I, [P, S, S]),
        "fa_lowrank_len": (S, [P, S, S, I]),
        "fa_lowrank_decode": (I, [P, S, S, P, I, U64, S, P]),
        "fa_lowrank_plan_bytes": (S, [P, S, S, U64, S]),
        "fa_lowrank_plan_build": (I, [P, S, S, U64, S, P, S]),
        "fa_lowrank_expand_device": (I, [P, I, P, S, P, I, U64, S, P, I, P, I, P]),
        "fa_set_lowrank": (I, [P, I, P, S, I]),
        "fa_submit_lowrank": (I, [P, I, I, P, S, I, F, I]),
        "fa_rot1_words": (S, [S]),
        "fa_rot1_blocks": (S, [S]),
        "fa_rot1_encode": (I, [P, S, U64, P, P]),
        "fa_rot1_decode": (I, [P, P, U64, U64, S, P]),
        "fa_rot1_expand_device": (I, [P, I, P, P, U64, U64, S, P, I, P, I, P]),
        "fa_rot1_encode_device": (I, [P, I, P, I, P, I, S, U64, U64, P, P, P, P]),
        "fa_set_rot1": (I, [P, I, I]),
        "fa_submit_rot1": (I, [P, I, I, P, P, U64, F, I]),
        "fa_set_secagg": (I, [P, I, F]),
        "fa_secagg_set_terms": (I, [P, I, I, P, P, P]),
        "fa_secagg_unmask_device": (I, [P, I, P, I, S, U64, I, P, P, P, F, P, I, P]),
        "fa_secagg_mask_host": (I, [P, P, U64, S, P]),
        "fa_secagg_quantize": (I, [P, S, F, P, ctypes.POINTER(U64)]),
        "fa_secagg_form": (I, [S, I]),
        "fa_sign_words": (S, [S]),
        "fa_sign_pack": (I, [P, S, P]),
        "fa_sign_vote_host": (I, [P, I, S, U64, F, I, I, P, P, P, P]),
        "fa_sign_vote_device": (I, [P, I, P, I, S, U64, F, I, I, P, I, P, I, P, P, P]),
        "fa_sign_form": (I, [S, P, I, U64, P, I, P, I, P, P]),
        "fa_set_sign": (I, [P, I, F, I, I, I]),
        "fa_submit_sign": (I, [P, I, I, P, I]),
        "fa_copy_sign_planes": (I, [P, I, P, P]),
        "fa_sparse_sum_host": (I, [P, P, P, P, I, S, U64, P, P]),
        "fa_sparse_sum_workspace": (S, [S, I]),
        "fa_sparse_sum_device": (I, [P, I, P, P, P, P, I, S, U64, P, I, P, I, P, P]),
        "fa_diag_sparse_sum": (I, [P, I, P, P, P, P, I, S, U64, P, I, P, I, P, I, P]),  # diagnostic (outside fa.h)
        "fa_sparse_sum_form": (I, [S, P, I, P, I, P, I]),
        "fa_set_sparse_sum": (I, [P, I, S]),
        "fa_submit_sparse": (I, [P, I, I, P, P, S, F, I]),
        "fa_mx8_sum_host": (I, [P, P, P, I, S, U64, P, P]),
        "fa_mx8_sum_device": (I, [P, I, P, P, P, I, S, U64, P, I, P, I, P]),
        "fa_mx8_sum_form": (I, [S, P, I, U64, P, I, P, I]),
        "fa_set_mx8_sum": (I, [P, I, I]),
        "fa_submit_mx8_sum": (I, [P, I, I, P, P, F, I]),
        "fa_lowrank_sum_host": (I, [P, S, S, P, P, P, I, U64, S, P, P]),
        "fa_lowrank_sum_device": (I, [P, I, P, S, P, P, P, I, U64, S, P, I, P, I, P]),
        "fa_set_lowrank_sum": (I, [P, I, P, S, I]),
        "fa_submit_lowrank_sum": (I, [P, I, I, P, S, I, F, I]),
        "fa_rot1_sum_host": (I, [P, P, P, P, I, U64, S, P, P]),
        "fa_rot1_sum_device": (I, [P, I, P, P, P, P, I, U64, S, P, I, P, I, P]),
        "fa_set_rot1_sum": (I, [P, I, I]),
        "fa_submit_rot1_sum": (I, [P, I, I, P, P, U64, F, I]),
        "fa_diag_secagg_unmask": (I, [P, I, P, I, S, U64, I, P, P, P, F, P, I, I, P]),  # diagnostic (outside fa.h)
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


def gram_device(clients, n, in_dtype, ref=None, stream=None, gpu=0, ctx=None):
    """fa_gram_device: the Gram matrix G_ab = sum_i y_a,i y_b,i (np.float64, shape (D, D), bit-symmetric, the
    diagonal the squared norms) of D device-resident client buckets, y the widened input or, with the fp32 device
    reference `ref`, fl32(x - ref) (fa.h "Gram pass").  Enqueued on `stream` and waited for.  With n == 0 no device is
    touched and the matrix is zeros: the feature probe."""
    D = len(clients)
    arr = (ctypes.c_void_p * max(1, D))(*[_addr(c) for c in clients])
    g = np.empty((D, D), np.float64)
    check(lib().fa_gram_device(ctx.handle if ctx is not None else None, gpu, arr, D, n, in_dtype, _addr(ref),
                               g.ctypes.data, _stream(stream)))
    return g


def dnc_select(gram, drop, iters=32):
    """fa_dnc_select (host arithmetic, rules 2-7 of fa.h "DnC stage"): (scores float64[D], selected bool[D]) of the
    (D, D) Gram matrix with `drop` owners to remove and `iters` power iterations."""
    gram = np.ascontiguousarray(gram, np.float64)
    D = gram.shape[0] if gram.ndim == 2 else 0
    if gram.ndim != 2 or gram.shape[1] != D:
        raise ValueError("need a square matrix")
    scores, sel = np.empty(D, np.float64), np.empty(D, np.intc)
    ns = ctypes.c_int()
    check(lib().fa_dnc_select(gram.ctypes.data, D, int(drop), int(iters), scores.ctypes.data, sel.ctypes.data,
                              ctypes.byref(ns)))
    return scores, sel.astype(bool)


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


TOPK_ABSOLUTE = 0x2  # FA_TOPK_ABSOLUTE
TOPK_TILE = 4096  # the elements of a workgroup's tile in the top-k kernels (fa_topk.hip)


def topk_encode(delta, k):
    """fa_topk_encode (host arithmetic, fa.h "Top-k receipts" rules 2-5): the min(k, n) entries of the fp32 deltas with
    the largest magnitude as (idx uint32[k'], val float32[k']), ascending in idx."""
    delta = np.ascontiguousarray(np.asarray(delta, np.float32).reshape(-1))
    kp = min(int(k), delta.size)
    idx, val, k_out = np.empty(kp, np.uint32), np.empty(kp, np.float32), ctypes.c_size_t(0)
    check(lib().fa_topk_encode(delta.ctypes.data, delta.size, int(k), idx.ctypes.data, val.ctypes.data, ctypes.byref(k_out)))
    return idx[:k_out.value], val[:k_out.value]


def topk_decode(idx, val, n, idx0=0):
    """fa_topk_decode (host arithmetic): the fp32 deltas of bucket elements idx0 .. idx0 + n - 1, +0 where no entry
    lies; entries outside the range are skipped, idx that is not strictly ascending is refused."""
    idx = np.ascontiguousarray(np.asarray(idx, np.uint32).reshape(-1))
    val = np.ascontiguousarray(np.asarray(val, np.float32).reshape(-1))
    if idx.size != val.size:
        raise ValueError("%d indices and %d values" % (idx.size, val.size))
    d = np.empty(n, np.float32)
    check(lib().fa_topk_decode(idx.ctypes.data, val.ctypes.data, idx.size, int(idx0), n, d.ctypes.data))
    return d


def topk_expand_device(idx, val, k, n, dst, dst_dtype=F32, ref=None, ref_dtype=F32, idx0=0, stream=None, gpu=0, ctx=None):
    """fa_topk_expand_device: dst[i] = ref[i] + d_i over n device-resident elements, bucket elements idx0 .. (ref None:
    absolute mode, dst[i] = d_i), from the k device-resident entries (idx, val), of which those outside the range are
    ignored.  Enqueued, not synchronized.  With n == 0 no device is touched: the feature probe."""
    check(lib().fa_topk_expand_device(ctx.handle if ctx is not None else None, gpu, _addr(idx), _addr(val), int(k), n,
                                      int(idx0), _addr(ref), ref_dtype, _addr(dst), dst_dtype, _stream(stream)))


def topk_encode_workspace(n):
    """fa_topk_encode_workspace: the bytes of topk_encode_device's scratch for n elements."""
    return lib().fa_topk_encode_workspace(n)


def topk_encode_device(new, sent, n, k, idx, val, work, out=None, dtype=F32, sent_dtype=None, stream=None, gpu=0,
                       ctx=None):
    """fa_topk_encode_device (fa.h "Top-k receipts", rules 1-6): over n device-resident elements of `dtype`, the
    min(k, n) entries of fl(new - sent) into idx and val, and (out not None) g' = sent + decode(idx, val) into out, which
    may be `sent` or `new` itself.  work: topk_encode_workspace(n) bytes of device scratch.  Enqueued, not synchronized.
    With n == 0 no device is touched: the feature probe."""
    check(lib().fa_topk_encode_device(ctx.handle if ctx is not None else None, gpu, _addr(new), dtype, _addr(sent),
                                      dtype if sent_dtype is None else sent_dtype, n, int(k), _addr(idx), _addr(val),
                                      _addr(out), _addr(work), _stream(stream)))


ROT1_ABSOLUTE = 0x2  # FA_ROT1_ABSOLUTE
ROT1_BLOCK = 4096  # FA_ROT1_BLOCK: elements per scale of a rot1 receipt (fa.h "Rot1 receipts")


def rot1_blocks(n):
    """fa_rot1_blocks: ceil(n / 4096), the scales of a rot1 receipt; its bits are 128 uint32 words per block."""
    return lib().fa_rot1_blocks(n)


def rot1_encode(delta, seed):
    """fa_rot1_encode (host arithmetic, fa.h "Rot1 receipts" rules 2-5): the fp32 deltas of a whole bucket as (bits
    uint32[128 nb], scale float32[nb])."""
    delta = np.ascontiguousarray(np.asarray(delta, np.float32).reshape(-1))
    nb = rot1_blocks(delta.size)
    bits, scale = np.empty(nb * 128, np.uint32), np.empty(nb, np.float32)
    check(lib().fa_rot1_encode(delta.ctypes.data, delta.size, int(seed), bits.ctypes.data, scale.ctypes.data))
    return bits, scale


def rot1_decode(bits, scale, seed, n, idx0=0):
    """fa_rot1_decode (host arithmetic): the fp32 deltas of bucket elements idx0 .. idx0 + n - 1; bits and scale start at
    block idx0 >> 12."""
    bits = np.ascontiguousarray(np.asarray(bits, np.uint32).reshape(-1))
    scale = np.ascontiguousarray(np.asarray(scale, np.float32).reshape(-1))
    nb = ((idx0 + n - 1) >> 12) - (idx0 >> 12) + 1 if n else 0
    if bits.size < nb * 128 or scale.size < nb:
        raise ValueError("elements [%d, %d) touch %d blocks, got %d words and %d scales" % (idx0, idx0 + n, nb, bits.size, scale.size))
    d = np.empty(n, np.float32)
    check(lib().fa_rot1_decode(bits.ctypes.data, scale.ctypes.data, int(seed), int(idx0), n, d.ctypes.data))
    return d


def rot1_expand_device(bits, scale, seed, n, dst, dst_dtype=F32, ref=None, ref_dtype=F32, idx0=0, stream=None, gpu=0,
                       ctx=None):
    """fa_rot1_expand_device: dst[i] = ref[i] + d_i over n device-resident elements, bucket elements idx0 .. (ref None:
    absolute mode, dst[i] = d_i), from the device-resident bits and scales of the blocks the range touches, block
    idx0 >> 12 first.  Enqueued, not synchronized.  With n == 0 no device is touched: the feature probe."""
    check(lib().fa_rot1_expand_device(ctx.handle if ctx is not None else None, gpu, _addr(bits), _addr(scale), int(seed),
                                      int(idx0), n, _addr(ref), ref_dtype, _addr(dst), dst_dtype, _stream(stream)))


def rot1_encode_device(new, sent, n, seed, bits, scale, out=None, dtype=F32, sent_dtype=None, idx0=0, stream=None, gpu=0,
                       ctx=None):
    """fa_rot1_encode_device (fa.h "Rot1 receipts", rules 1-6): over n device-resident elements of `dtype`, bucket
    elements idx0 .. (a multiple of 4096), the bits and scales of fl(new - sent), and (out not None) g' = sent +
    decode(bits, scale) into out, which may be `sent` or `new` itself.  Enqueued, not synchronized.  With n == 0 no device
    is touched: the feature probe."""
    check(lib().fa_rot1_encode_device(ctx.handle if ctx is not None else None, gpu, _addr(new), dtype, _addr(sent),
                                      dtype if sent_dtype is None else sent_dtype, n, int(idx0), int(seed), _addr(bits),
                                      _addr(scale), _addr(out), _stream(stream)))


LOWRANK_ABSOLUTE = 0x2  # FA_LOWRANK_ABSOLUTE
LOWRANK_MAX_RANK = 64  # FA_LOWRANK_MAX_RANK
LOWRANK_MAT = np.dtype([("off", np.uint64), ("rows", np.uint32), ("cols", np.uint32)])  # fa_lowrank_mat


def _lowrank_table(mats):
    """A table as a contiguous array of fa_lowrank_mat: a LOWRANK_MAT array, or rows of (off, rows, cols)."""
    if isinstance(mats, np.ndarray) and mats.dtype == LOWRANK_MAT:
        return np.ascontiguousarray(mats.reshape(-1))
    t = np.zeros(len(mats), LOWRANK_MAT)
    for j, (off, rows, cols) in enumerate(mats):
        t[j] = (off, rows, cols)
    return t


def lowrank_mats(shapes, min_elems=0):
    """A table from a list of tensor shapes laid out back to back, as named_parameters() flattens them: [shape[0],
    prod(shape[1:])] for tensors of at least two dimensions and min_elems elements; the others are rest.  Returns (table,
    n)."""
    rows, off = [], 0
    for shape in shapes:
        size = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        if len(shape) >= 2 and size >= max(1, min_elems):
            rows.append((off, int(shape[0]), size // int(shape[0])))
        off += size
    return _lowrank_table(rows), off


def lowrank_check(mats, n):
    """fa_lowrank_check: FaError(ERR_ARG) naming the first entry that breaks the table rules for a bucket of n elements."""
    t = _lowrank_table(mats)
    check(lib().fa_lowrank_check(t.ctypes.data, t.size, n))


def lowrank_len(mats, n, r):
    """fa_lowrank_len: the fp32 values of a receipt of rank r over the table: r * sum (rows + cols) + |rest|."""
    t = _lowrank_table(mats)
    size = lib().fa_lowrank_len(t.ctypes.data, t.size, n, int(r))
    if size == 0:
        err = lib().fa_last_error().decode(errors="replace")
        if err:
            raise FaError(ERR_ARG, err)
    return size


def lowrank_decode(f, mats, n, r, idx0=0, cnt=None):
    """fa_lowrank_decode (host arithmetic, fa.h "Low-rank receipts"): the fp32 deltas of bucket elements idx0 .. idx0 +
    cnt - 1 (cnt None: to the end) from the receipt f of rank r."""
    t = _lowrank_table(mats)
    f = np.ascontiguousarray(np.asarray(f, np.float32).reshape(-1))
    if f.size != lowrank_len(t, n, r):
        raise ValueError("%d values, a receipt of rank %d has %d" % (f.size, r, lowrank_len(t, n, r)))
    cnt = n - idx0 if cnt is None else cnt
    d = np.empty(cnt, np.float32)
    check(lib().fa_lowrank_decode(t.ctypes.data, t.size, n, f.ctypes.data, int(r), int(idx0), cnt, d.ctypes.data))
    return d


def lowrank_plan(mats, n, idx0=0, cnt=None):
    """fa_lowrank_plan_bytes / fa_lowrank_plan_build: the plan of one launch over bucket elements [idx0, idx0 + cnt) as a
    uint8 array, for the caller to put into device memory."""
    t = _lowrank_table(mats)
    cnt = n - idx0 if cnt is None else cnt
    size = lib().fa_lowrank_plan_bytes(t.ctypes.data, t.size, n, int(idx0), cnt)
    if size == 0:
        raise FaError(ERR_ARG, lib().fa_last_error().decode(errors="replace"))
    plan = np.zeros(size, np.uint8)
    check(lib().fa_lowrank_plan_build(t.ctypes.data, t.size, n, int(idx0), cnt, plan.ctypes.data, size))
    return plan


def lowrank_expand_device(plan, f, r, cnt, dst, dst_dtype=F32, ref=None, ref_dtype=F32, idx0=0, plan_bytes=None,
                          stream=None, gpu=0, ctx=None):
    """fa_lowrank_expand_device: dst[i] = ref[i] + d_i over cnt device-resident elements, bucket elements idx0 .. (ref
    None: absolute mode, dst[i] = d_i), from the device-resident receipt f of rank r and the device-resident plan of
    exactly that range (lowrank_plan).  Enqueued, not synchronized.  With cnt == 0 no device is touched: the feature
    probe."""
    if plan_bytes is None:
        plan_bytes = plan.numel() * plan.element_size() if hasattr(plan, "numel") else getattr(plan, "nbytes", 0)
    check(lib().fa_lowrank_expand_device(ctx.handle if ctx is not None else None, gpu, _addr(plan), int(plan_bytes),
                                         _addr(f), int(r), int(idx0), cnt, _addr(ref), ref_dtype, _addr(dst), dst_dtype,
                                         _stream(stream)))


LOWRANK_SUM_MAX_CLIENTS = 128  # FA_LOWRANK_SUM_MAX_CLIENTS


ROT1_SUM_MAX_CLIENTS = 128  # FA_ROT1_SUM_MAX_CLIENTS
ROT1_SUM_DEPTH = 8  # the owners whose half-words a lane keeps in flight


def _rot1_sum_args(bits, scale, seed, weights):
    """The pointer arrays, the seeds (one per owner, or one for all) and the weights of D receipts (bits[c], scale[c]).
    Returns ctypes and numpy arrays, which the caller keeps until the call returns."""
    D = len(bits)
    if len(scale) != D:
        raise ValueError("need one scale per bits")
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, np.uint64).reshape(-1), (D,)) if np.size(seed) == 1
                              else np.asarray(seed, np.uint64).reshape(-1))
    w = np.ascontiguousarray(np.ones(D) if weights is None else weights, np.float32).reshape(-1)
    if w.size != D or sd.size != D:
        raise ValueError("need one weight and one seed per client")
    pb = (ctypes.c_void_p * max(1, D))(*[_addr(x) for x in bits])
    ps = (ctypes.c_void_p * max(1, D))(*[_addr(x) for x in scale])
    return pb, ps, sd, w, D


def rot1_sum_host(bits, scale, seed, n, weights=None, ref=None, idx0=0):
    """fa_rot1_sum_host (host arithmetic, fa.h "Rot1-sum stage" rules 0-6): the fp32 aggregate of bucket elements idx0 ..
    idx0 + n - 1 from the receipts (bits[c] uint32, scale[c] float32, both from block idx0 >> 12 on; seed: one per owner
    or one for all) under `weights` (None: ones) and ref (fp32[n], None: absolute mode)."""
    bits = [np.ascontiguousarray(np.asarray(x, np.uint32).reshape(-1)) for x in bits]
    scale = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in scale]
    nb = ((int(idx0) + n - 1) >> 12) - (int(idx0) >> 12) + 1 if n else 0
    if any(x.size < nb * 128 for x in bits) or any(x.size < nb for x in scale):
        raise ValueError("need %d words and %d scales per client" % (nb * 128, nb))
    pb, ps, sd, w, D = _rot1_sum_args(bits, scale, seed, weights)
    if ref is not None:
        ref = np.ascontiguousarray(np.asarray(ref, np.float32).reshape(-1))
    out = np.empty(n, np.float32)
    check(lib().fa_rot1_sum_host(pb, ps, sd.ctypes.data, w.ctypes.data, D, int(idx0), n, _addr(ref), out.ctypes.data))
    return out


def rot1_sum_device(bits, scale, seed, n, out, out_dtype=F32, weights=None, ref=None, ref_dtype=F32, idx0=0, stream=None,
                    gpu=0, ctx=None):
    """fa_rot1_sum_device: out[i] = ref[i] + acc_i (ref None: acc_i) over n device-resident elements, bucket elements
    idx0 .., from the D device-resident receipts (bits[c], scale[c]), bits / scale / idx0 as for rot1_expand_device, at any
    element phase of ref and out.  Enqueued, not synchronized.  With n == 0 no device is touched: the feature probe."""
    pb, ps, sd, w, D = _rot1_sum_args(bits, scale, seed, weights)
    check(lib().fa_rot1_sum_device(ctx.handle if ctx is not None else None, gpu, pb, ps, sd.ctypes.data, w.ctypes.data, D,
                                   int(idx0), n, _addr(ref), ref_dtype, _addr(out), out_dtype, _stream(stream)))


def _lowrank_sum_args(f, r, weights):
    """The pointer array, the ranks and the weights of D receipts f[c] of rank r[c].  Returns arrays the caller keeps until
    the call returns."""
    D = len(f)
    r = np.ascontiguousarray(r, np.int32).reshape(-1)
    w = np.ascontiguousarray(np.ones(D) if weights is None else weights, np.float32).reshape(-1)
    if r.size != D or w.size != D:
        raise ValueError("need one rank and one weight per client")
    return (ctypes.c_void_p * max(1, D))(*[_addr(x) for x in f]), r, w, D


def lowrank_sum_host(f, r, mats, n, weights=None, ref=None, idx0=0, cnt=None):
    """fa_lowrank_sum_host (host arithmetic, fa.h "Low-rank-sum stage" rules 1-4): the fp32 aggregate of bucket elements
    idx0 .. idx0 + cnt - 1 (cnt None: to the end) from the receipts f[c] of rank r[c] under `weights` (None: ones) and
    ref (fp32[cnt], None: absolute mode)."""
    t = _lowrank_table(mats)
    f = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in f]
    for x, rc in zip(f, r):
        if x.size != lowrank_len(t, n, rc):
            raise ValueError("%d values, a receipt of rank %d has %d" % (x.size, rc, lowrank_len(t, n, rc)))
    pf, r, w, D = _lowrank_sum_args(f, r, weights)
    cnt = n - idx0 if cnt is None else cnt
    if ref is not None:
        ref = np.ascontiguousarray(np.asarray(ref, np.float32).reshape(-1))
    out = np.empty(cnt, np.float32)
    check(lib().fa_lowrank_sum_host(t.ctypes.data, t.size, n, pf, r.ctypes.data, w.ctypes.data, D, int(idx0), cnt, _addr(ref),
                                    out.ctypes.data))
    return out


def lowrank_sum_device(plan, f, r, cnt, out, out_dtype=F32, weights=None, ref=None, ref_dtype=F32, idx0=0, plan_bytes=None,
                       stream=None, gpu=0, ctx=None):
    """fa_lowrank_sum_device: out[i] = ref[i] + acc_i (ref None: acc_i) over cnt device-resident elements, bucket elements
    idx0 .., from the D device-resident receipts f[c] of rank r[c] under `weights` and the device-resident plan of exactly
    that range (lowrank_plan).  Enqueued, not synchronized.  With cnt == 0 no device is touched: the feature probe."""
    if plan_bytes is None:
        plan_bytes = plan.numel() * plan.element_size() if hasattr(plan, "numel") else getattr(plan, "nbytes", 0)
    pf, r, w, D = _lowrank_sum_args(f, r, weights)
    check(lib().fa_lowrank_sum_device(ctx.handle if ctx is not None else None, gpu, _addr(plan), int(plan_bytes), pf,
                                      r.ctypes.data, w.ctypes.data, D, int(idx0), cnt, _addr(ref), ref_dtype, _addr(out),
                                      out_dtype, _stream(stream)))


def lowrank_encode(delta, mats, r):
    """The owner's side in numpy, not specified bit for bit (any f is valid input): per matrix of the table a rank-r
    truncated SVD of its block of the fp32 deltas, P = U_r S_r and Q = V_r (zero columns beyond the matrix's own rank),
    then the rest elements copied.  LoRA owners bring their own factors instead."""
    t = _lowrank_table(mats)
    delta = np.ascontiguousarray(np.asarray(delta, np.float32).reshape(-1))
    lowrank_check(t, delta.size)
    covered = np.zeros(delta.size, bool)
    out = []
    for off, rows, cols in t.tolist():
        covered[off:off + rows * cols] = True
        u, s, vt = np.linalg.svd(delta[off:off + rows * cols].reshape(rows, cols).astype(np.float64), full_matrices=False)
        p, q = np.zeros((rows, r), np.float32), np.zeros((cols, r), np.float32)
        k = min(r, s.size)
        p[:, :k] = u[:, :k] * s[:k]
        q[:, :k] = vt[:k].T
        out += [p.reshape(-1), q.reshape(-1)]
    return np.concatenate(out + [delta[~covered]]).astype(np.float32)


SECAGG_MAX_TERMS = 4096  # FA_SECAGG_MAX_TERMS
SECAGG_TILE, SECAGG_SPLIT = 0, 1  # secagg_form


def _secagg_terms(keys, nonces, signs):
    """(T, keys uint32[T, 8], nonces uint32[T, 3], signs intc[T]) as contiguous arrays."""
    keys = np.ascontiguousarray(np.asarray(keys, np.uint32).reshape(-1, 8))
    nonces = np.ascontiguousarray(np.asarray(nonces, np.uint32).reshape(-1, 3))
    signs = np.ascontiguousarray(np.asarray(signs, np.intc).reshape(-1))
    if not keys.shape[0] == nonces.shape[0] == signs.size:
        raise ValueError("need one key, one nonce and one sign per term")
    return signs.size, keys, nonces, signs


def secagg_unmask_device(clients, n, out, out_dtype=F32, keys=(), nonces=(), signs=(), scale=1.0, idx0=0, form=None,
                         stream=None, gpu=0, ctx=None):
    """fa_secagg_unmask_device (fa.h "Secagg stage", rules 2-4): out[i] = (int32)(the sum modulo 2^32 of the D
    device-resident uint32 buckets and the signed ChaCha20 words of the terms at bucket element idx0 + i) * scale, in
    out_dtype.  Enqueued on `stream` and waited for.  form: None, or SECAGG_TILE / SECAGG_SPLIT to force a vector form
    (the diagnostic entry; the same bits).  With n == 0 no device is touched: the feature probe."""
    D = len(clients)
    arr = (ctypes.c_void_p * max(1, D))(*[_addr(c) for c in clients])
    T, keys, nonces, signs = _secagg_terms(keys, nonces, signs)
    args = [ctx.handle if ctx is not None else None, gpu, arr, D, n, int(idx0), T, keys.ctypes.data, nonces.ctypes.data,
            signs.ctypes.data, float(scale), _addr(out), out_dtype]
    if form is None:
        check(lib().fa_secagg_unmask_device(*args, _stream(stream)))
    else:
        check(lib().fa_diag_secagg_unmask(*args, int(form), _stream(stream)))


def secagg_mask_host(key, nonce, idx0, n):
    """fa_secagg_mask_host (host arithmetic): the n mask words (np.uint32) of bucket elements idx0 .. idx0 + n - 1 under
    key (8 words) and nonce (3 words): the owner's side, and the bits the kernel removes."""
    key = np.ascontiguousarray(np.asarray(key, np.uint32).reshape(8))
    nonce = np.ascontiguousarray(np.asarray(nonce, np.uint32).reshape(3))
    out = np.empty(n, np.uint32)
    check(lib().fa_secagg_mask_host(key.ctypes.data, nonce.ctypes.data, int(idx0), n, out.ctypes.data))
    return out


def secagg_quantize(v, q):
    """fa_secagg_quantize (host arithmetic, the owner's side): (codes int32[n], n_bad) -- rint(v * q) in fp64, ties to
    even, saturated at +-(2^31 - 1); a NaN gives 0 and is counted."""
    v = np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1))
    out, bad = np.empty(v.size, np.int32), ctypes.c_uint64()
    check(lib().fa_secagg_quantize(v.ctypes.data, v.size, float(q), out.ctypes.data, ctypes.byref(bad)))
    return out, bad.value


def secagg_form(n, T):
    """fa_secagg_form (host arithmetic): SECAGG_TILE or SECAGG_SPLIT, the vector form a launch over n elements and T
    terms takes."""
    return lib().fa_secagg_form(n, int(T))


SIGN_MAX_CLIENTS = 128  # FA_SIGN_MAX_CLIENTS
SIGN_MAJORITY, SIGN_MEAN = 0, 1  # FA_SIGN_MAJORITY, FA_SIGN_MEAN
SIGN_ELEMENT, SIGN_VECTOR = 0, 1  # sign_form


def sign_words(n):
    """fa_sign_words: ceil(n / 32), the uint32 words of a sign receipt and of a vote plane of n elements."""
    return lib().fa_sign_words(n)


def sign_pack(delta):
    """fa_sign_pack (host arithmetic, fa.h "Sign-vote stage" rule 2): the sign receipt (np.uint32 words) of the fp32
    deltas of a whole bucket: the bit is set iff delta < 0."""
    delta = np.ascontiguousarray(np.asarray(delta, np.float32).reshape(-1))
    bits = np.empty(sign_words(delta.size), np.uint32)
    check(lib().fa_sign_pack(delta.ctypes.data, delta.size, bits.ctypes.data))
    return bits


def _sign_ptrs(bits):
    return (ctypes.c_void_p * max(1, len(bits)))(*[_addr(b) for b in bits])


def sign_vote_host(bits, n, eta, rule=SIGN_MAJORITY, margin=1, ref=None, idx0=0, planes=False):
    """fa_sign_vote_host (host arithmetic, rules 3-9): the fp32 aggregate of bucket elements idx0 .. idx0 + n - 1 from the
    whole receipts `bits` (np.uint32 arrays) and ref (fp32[n], None: absolute mode); with planes (a, neg, pos)."""
    bits = [np.ascontiguousarray(np.asarray(b, np.uint32).reshape(-1)) for b in bits]
    if ref is not None:
        ref = np.ascontiguousarray(np.asarray(ref, np.float32).reshape(-1))
    out = np.empty(n, np.float32)
    neg, pos = (np.empty(sign_words(n), np.uint32), np.empty(sign_words(n), np.uint32)) if planes else (None, None)
    check(lib().fa_sign_vote_host(_sign_ptrs(bits), len(bits), n, int(idx0), float(eta), int(rule), int(margin), _addr(ref),
                                  out.ctypes.data, _addr(neg), _addr(pos)))
    return (out, neg, pos) if planes else out


def sign_vote_device(bits, n, out, out_dtype=F32, eta=1.0, rule=SIGN_MAJORITY, margin=1, ref=None, ref_dtype=F32, idx0=0,
                     neg=None, pos=None, stream=None, gpu=0, ctx=None):
    """fa_sign_vote_device: out[i] = ref[i] + t_i (ref None: t_i) over n device-resident elements, bucket elements idx0 ..,
    from the D device-resident whole receipts `bits`; neg, pos: the vote planes (sign_words(n) uint32 words each).
    Enqueued, not synchronized.  With n == 0 no device is touched: the feature probe."""
    check(lib().fa_sign_vote_device(ctx.handle if ctx is not None else None, gpu, _sign_ptrs(bits), len(bits), n, int(idx0),
                                    float(eta), int(rule), int(margin), _addr(ref), ref_dtype, _addr(out), out_dtype,
                                    _addr(neg), _addr(pos), _stream(stream)))


def sign_form(n, bits, out, out_dtype=F32, ref=None, ref_dtype=F32, idx0=0, neg=None, pos=None):
    """fa_sign_form (host arithmetic on the addresses): SIGN_VECTOR if sign_vote_device takes the vector form for these
    operands, SIGN_ELEMENT if the element form throughout."""
    rc = lib().fa_sign_form(n, _sign_ptrs(bits), len(bits), int(idx0), _addr(ref), ref_dtype, _addr(out), out_dtype,
                            _addr(neg), _addr(pos))
    return rc if rc >= 0 else check(rc)


SPARSE_MAX_CLIENTS = 128  # FA_SPARSE_MAX_CLIENTS
SPARSE_VECTOR, SPARSE_BIG_TILE = 1, 2  # sparse_sum_form: a bit each
SPARSE_TILES = (2048, 8192)  # the elements a wave owns: the small tile, the big one (densities below 1 / 2048)
SPARSE_GROUP = 4  # the clients whose first entries a wave keeps in flight


def _sparse_args(idx, val, k, weights):
    """The pointer arrays, the counts and the weights of D receipts (idx[c], val[c]) of k[c] entries.  Returns ctypes
    arrays, which the caller keeps until the call returns."""
    D = len(idx)
    if len(val) != D or len(k) != D:
        raise ValueError("need one val and one count per idx")
    w = np.ascontiguousarray(np.ones(D) if weights is None else weights, np.float32).reshape(-1)
    if w.size != D:
        raise ValueError("need one weight per client")
    pi = (ctypes.c_void_p * max(1, D))(*[_addr(x) for x in idx])
    pv = (ctypes.c_void_p * max(1, D))(*[_addr(x) for x in val])
    return pi, pv, (ctypes.c_size_t * max(1, D))(*[int(x) for x in k]), w, D


def sparse_sum_host(idx, val, n, weights=None, ref=None, idx0=0):
    """fa_sparse_sum_host (host arithmetic, fa.h "Sparse-sum stage" rules 1-2): the fp32 aggregate of bucket elements idx0 ..
    idx0 + n - 1 from the receipts (idx[c] np.uint32 ascending, val[c] np.float32) under `weights` (None: ones) and ref
    (fp32[n], None: absolute mode)."""
    idx = [np.ascontiguousarray(np.asarray(i, np.uint32).reshape(-1)) for i in idx]
    val = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1)) for v in val]
    if [i.size for i in idx] != [v.size for v in val]:
        raise ValueError("idx and val differ in length")
    pi, pv, k, w, D = _sparse_args(idx, val, [v.size for v in val], weights)
    if ref is not None:
        ref = np.ascontiguousarray(np.asarray(ref, np.float32).reshape(-1))
    out = np.empty(n, np.float32)
    check(lib().fa_sparse_sum_host(pi, pv, k, w.ctypes.data, D, n, int(idx0), _addr(ref), out.ctypes.data))
    return out


def sparse_sum_workspace(n, D):
    """fa_sparse_sum_workspace: the bytes of sparse_sum_device's scratch for n elements and D clients."""
    return lib().fa_sparse_sum_workspace(n, int(D))


def sparse_sum_device(idx, val, k, n, out, work, out_dtype=F32, weights=None, ref=None, ref_dtype=F32, idx0=0, tile=None,
                      stream=None, gpu=0, ctx=None):
    """fa_sparse_sum_device: out[i] = ref[i] + sum_c w_c d_c,i (ref None: the sum) over n device-resident elements, bucket
    elements idx0 .., from the D device-resident receipts (idx[c], val[c]) of k[c] entries; work: sparse_sum_workspace(n, D) bytes of device
    scratch.  tile: None, or 0 / 1 to force the small / the big tile (the diagnostic entry; the same bits).  Enqueued, not
    synchronized.  With n == 0 no device is touched: the feature probe."""
    pi, pv, k, w, D = _sparse_args(idx, val, k, weights)
    args = [ctx.handle if ctx is not None else None, gpu, pi, pv, k, w.ctypes.data, D, n, int(idx0), _addr(ref), ref_dtype,
            _addr(out), out_dtype, _addr(work)]
    if tile is None:
        check(lib().fa_sparse_sum_device(*args, _stream(stream)))
    else:
        check(lib().fa_diag_sparse_sum(*args, int(tile), _stream(stream)))


def sparse_sum_form(n, k, out, out_dtype=F32, ref=None, ref_dtype=F32):
    """fa_sparse_sum_form (host arithmetic on the counts k and the addresses): SPARSE_VECTOR if the dense side of
    sparse_sum_device takes 16-byte accesses for these operands, SPARSE_BIG_TILE if a wave owns the big tile."""
    kk = (ctypes.c_size_t * max(1, len(k)))(*[int(x) for x in k])
    rc = lib().fa_sparse_sum_form(n, kk, len(k), _addr(ref), ref_dtype, _addr(out), out_dtype)
    return rc if rc >= 0 else check(rc)


MX8_SUM_MAX_CLIENTS = 128  # FA_MX8_SUM_MAX_CLIENTS
MX8_SUM_VECTOR = 1  # mx8_sum_form
MX8_SUM_TILE = 4096  # the elements of a workgroup's tile: 128 blocks, 16 elements per lane
MX8_SUM_GROUP = 4  # the clients whose q words a lane keeps in flight


def _mx8_sum_args(q, e, weights):
    """The pointer arrays and the weights of D receipts (q[c], e[c]).  Returns ctypes arrays, which the caller keeps until
    the call returns."""
    D = len(q)
    if len(e) != D:
        raise ValueError("need one e per q")
    w = np.ascontiguousarray(np.ones(D) if weights is None else weights, np.float32).reshape(-1)
    if w.size != D:
        raise ValueError("need one weight per client")
    pq = (ctypes.c_void_p * max(1, D))(*[_addr(x) for x in q])
    pe = (ctypes.c_void_p * max(1, D))(*[_addr(x) for x in e])
    return pq, pe, w, D


def mx8_sum_host(q, e, n, weights=None, ref=None, idx0=0):
    """fa_mx8_sum_host (host arithmetic, fa.h "MX8-sum stage" rules 1-3): the fp32 aggregate of bucket elements idx0 .. idx0 +
    n - 1 from the receipts (q[c] int8[n], e[c] uint8, e[c][0] the scale of element idx0's block) under `weights` (None:
    ones) and ref (fp32[n], None: absolute mode)."""
    q = [np.ascontiguousarray(np.asarray(x, np.int8).reshape(-1)) for x in q]
    e = [np.ascontiguousarray(np.asarray(x, np.uint8).reshape(-1)) for x in e]
    blocks = ((int(idx0) + n - 1) >> 5) - (int(idx0) >> 5) + 1 if n else 0
    if any(x.size != n for x in q) or any(x.size < blocks for x in e):
        raise ValueError("need %d codes and %d scales per client" % (n, blocks))
    pq, pe, w, D = _mx8_sum_args(q, e, weights)
    if ref is not None:
        ref = np.ascontiguousarray(np.asarray(ref, np.float32).reshape(-1))
    out = np.empty(n, np.float32)
    check(lib().fa_mx8_sum_host(pq, pe, w.ctypes.data, D, n, int(idx0), _addr(ref), out.ctypes.data))
    return out


def mx8_sum_device(q, e, n, out, out_dtype=F32, weights=None, ref=None, ref_dtype=F32, idx0=0, stream=None, gpu=0, ctx=None):
    """fa_mx8_sum_device: out[i] = ref[i] + sum_c w_c d_c,i (ref None: the sum) over n device-resident elements, bucket
    elements idx0 .., from the D device-resident receipts (q[c], e[c]), q / e / idx0 as for mx8_decode, at any byte (q, e)
    or element (ref, out) phase.  Enqueued, not synchronized.  With n == 0 no device is touched: the feature probe."""
    pq, pe, w, D = _mx8_sum_args(q, e, weights)
    check(lib().fa_mx8_sum_device(ctx.handle if ctx is not None else None, gpu, pq, pe, w.ctypes.data, D, n, int(idx0),
                                  _addr(ref), ref_dtype, _addr(out), out_dtype, _stream(stream)))


def mx8_sum_form(n, q, out, out_dtype=F32, ref=None, ref_dtype=F32, idx0=0):
    """fa_mx8_sum_form (host arithmetic on the addresses and idx0): MX8_SUM_VECTOR if mx8_sum_device takes a lane's 16
    elements in 16-byte accesses for these operands, 0 if it goes element by element."""
    pq = (ctypes.c_void_p * max(1, len(q)))(*[_addr(x) for x in q])
    rc = lib().fa_mx8_sum_form(n, pq, len(q), int(idx0), _addr(ref), ref_dtype, _addr(out), out_dtype)
    return rc if rc >= 0 else check(rc)


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

    def set_dnc(self, drop, iters=32, part_id=-1):
        """fa_set_dnc: DnC spectral selection on a FEDAVG part, removing the `drop` owners that project farthest on
        the top singular direction of the centred buckets, found by `iters` power iterations on the Gram matrix
        (part_id < 0: the default of FEDAVG parts defined later); iters=0 removes the stage."""
        check(lib().fa_set_dnc(self.handle, part_id, int(drop), int(iters)))

    def dnc_round(self, part_id):
        """fa_dnc_get_round: (gram float64[D, D], scores float64[D], selected bool[D]) of the part's last reducing
        call."""
        D = self.parts[part_id][3]
        g, s, sel = np.empty((D, D), np.float64), np.empty(D, np.float64), np.empty(D, np.intc)
        ns = ctypes.c_int()
        check(lib().fa_dnc_get_round(self.handle, part_id, g.ctypes.data, s.ctypes.data, sel.ctypes.data,
                                     ctypes.byref(ns)))
        return g, s, sel.astype(bool)

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

    def set_secagg(self, scale, part_id):
        """fa_set_secagg: the part's slots hold masked uint32 words (submit them as 4-byte elements: a uint32 array, or
        its float32 view); a reducing call sums them modulo 2^32, removes the round's terms and decodes with `scale`.
        scale <= 0 removes the stage."""
        check(lib().fa_set_secagg(self.handle, part_id, float(scale)))

    def secagg_terms(self, part_id, keys, nonces, signs):
        """fa_secagg_set_terms: the terms of the part's next reducing call -- keys uint32[T, 8], nonces uint32[T, 3],
        signs (+1 / -1)[T]; T = 0 (three empty sequences) is set explicitly."""
        T, keys, nonces, signs = _secagg_terms(keys, nonces, signs)
        check(lib().fa_secagg_set_terms(self.handle, part_id, T, keys.ctypes.data, nonces.ctypes.data, signs.ctypes.data))

    def set_sign(self, part, eta, rule=SIGN_MAJORITY, margin=1, planes=False):
        """fa_set_sign: the part's rounds are sign votes over one-bit receipts (submit_sign), a_i = g_i + t_i with g the
        part's last output; eta <= 0 removes the stage.  planes: the reducing calls leave the vote planes."""
        check(lib().fa_set_sign(self.handle, part, float(eta), int(rule), int(margin), 1 if planes else 0))

    def submit_sign(self, part, slot, bits, pinned=False):
        """fa_submit_sign: the client's sign receipt (uint32[sign_words(n)]).  pinned: a view of a PinnedBuffer the
        caller keeps unchanged until the round is reduced."""
        bits = np.ascontiguousarray(bits)
        if bits.dtype != np.uint32:
            raise ValueError("need bits uint32")
        if part in self.parts and bits.size != sign_words(self.parts[part][0]):
            raise ValueError("bucket %d expects %d words, got %d" % (part, sign_words(self.parts[part][0]), bits.size))
        check(lib().fa_submit_sign(self.handle, part, slot, bits.ctypes.data, HOST_PINNED if pinned else 0))

    def copy_sign_planes(self, part):
        """fa_copy_sign_planes: (neg, pos), the vote planes of the part's last reducing call (uint32[sign_words(n)])."""
        words = sign_words(self.parts[part][0]) if part in self.parts else 0
        neg, pos = np.empty(words, np.uint32), np.empty(words, np.uint32)
        check(lib().fa_copy_sign_planes(self.handle, part, neg.ctypes.data, pos.ctypes.data))
        return neg, pos

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

    def set_topk(self, k_max, part=None):
        """fa_set_topk: the part takes top-k receipts of at most k_max entries, on the stage and the reference of
        set_mx8 (part None: the default of parts defined later); 0 switches them off."""
        check(lib().fa_set_topk(self.handle, -1 if part is None else part, int(k_max)))

    def submit_topk(self, part, slot, idx, val, weight=1.0, absolute=False, pinned=False):
        """fa_submit_topk: the client's update against the part's last output as (idx uint32[k] ascending, val
        float32[k]), expanded into the slot on the GPU.  pinned: views of PinnedBuffers the caller keeps unchanged until
        finalize returns.  absolute: the values themselves, no reference."""
        idx, val = np.ascontiguousarray(idx), np.ascontiguousarray(val)
        if idx.dtype != np.uint32 or val.dtype != np.float32 or idx.size != val.size:
            raise ValueError("need idx uint32 and val float32 of one length")
        flags = (HOST_PINNED if pinned else 0) | (TOPK_ABSOLUTE if absolute else 0)
        check(lib().fa_submit_topk(self.handle, part, slot, idx.ctypes.data, val.ctypes.data, idx.size, float(weight), flags))

    def set_sparse_sum(self, part, k_max):
        """fa_set_sparse_sum: the part's rounds take top-k receipts of at most k_max entries (submit_sparse) and reduce them
        without expanding them, a_i = g_i + sum_c w_c d_c,i with g the part's last output; 0 removes the stage."""
        check(lib().fa_set_sparse_sum(self.handle, part, int(k_max)))

    def submit_sparse(self, part, slot, idx, val, weight=1.0, pinned=False):
        """fa_submit_sparse: the client's update as (idx uint32[k] ascending, val float32[k]), kept as it is until the
        reducing call.  pinned: views of PinnedBuffers the caller keeps unchanged until the round is reduced."""
        idx, val = np.ascontiguousarray(idx), np.ascontiguousarray(val)
        if idx.dtype != np.uint32 or val.dtype != np.float32 or idx.size != val.size:
            raise ValueError("need idx uint32 and val float32 of one length")
        check(lib().fa_submit_sparse(self.handle, part, slot, idx.ctypes.data, val.ctypes.data, idx.size, float(weight),
                                     HOST_PINNED if pinned else 0))

    def set_mx8_sum(self, on=True, part_id=-1):
        """fa_set_mx8_sum: the part's rounds take MX8 receipts (submit_mx8_sum) and reduce them without expanding them,
        a_i = g_i + sum_c w_c d_c,i with g the part's last output; on=False removes the stage."""
        check(lib().fa_set_mx8_sum(self.handle, part_id, 1 if on else 0))

    def submit_mx8_sum(self, part_id, slot, q, e, weight=1.0, pinned=False):
        """fa_submit_mx8_sum: the client's update as (q int8[n], e uint8[ceil(n / 32)]), kept as it is until the reducing
        call.  pinned: views of PinnedBuffers the caller keeps unchanged until the round is reduced."""
        q, e = np.ascontiguousarray(q), np.ascontiguousarray(e)
        if q.dtype != np.int8 or e.dtype != np.uint8:
            raise ValueError("need q int8 and e uint8")
        if part_id in self.parts:
            n = self.parts[part_id][0]
            if q.size != n or e.size != mx8_scale_bytes(n):
                raise ValueError("bucket %d expects %d codes and %d scales, got %d and %d"
                                 % (part_id, n, mx8_scale_bytes(n), q.size, e.size))
        check(lib().fa_submit_mx8_sum(self.handle, part_id, slot, q.ctypes.data, e.ctypes.data, float(weight),
                                      HOST_PINNED if pinned else 0))

    def set_lowrank(self, part, mats, r_max):
        """fa_set_lowrank: the part takes low-rank receipts of rank at most r_max over the table (lowrank_mats, or rows
        of (off, rows, cols)), on the stage and the reference of set_mx8; an empty table switches them off."""
        t = _lowrank_table(mats)
        check(lib().fa_set_lowrank(self.handle, part, t.ctypes.data, t.size, int(r_max)))

    def submit_lowrank(self, part, slot, f, r, weight=1.0, absolute=False, pinned=False):
        """fa_submit_lowrank: the client's update against the part's last output as the fp32 receipt f of rank r (per
        matrix P then Q, then the rest), expanded into the slot on the GPU.  pinned: a view of a PinnedBuffer the caller
        keeps unchanged until finalize returns.  absolute: the deltas themselves, no reference."""
        f = np.ascontiguousarray(f)
        if f.dtype != np.float32:
            raise ValueError("need f float32")
        flags = (HOST_PINNED if pinned else 0) | (LOWRANK_ABSOLUTE if absolute else 0)
        check(lib().fa_submit_lowrank(self.handle, part, slot, f.ctypes.data, f.size, int(r), float(weight), flags))

    def set_lowrank_sum(self, part, mats, r_max):
        """fa_set_lowrank_sum: the part's rounds take low-rank receipts of rank at most r_max over the table
        (submit_lowrank_sum) and reduce them as one stacked product, without expanding them; an empty table removes
        the stage."""
        t = _lowrank_table(mats)
        check(lib().fa_set_lowrank_sum(self.handle, part, t.ctypes.data, t.size, int(r_max)))

    def submit_lowrank_sum(self, part, slot, f, r, weight=1.0, pinned=False):
        """fa_submit_lowrank_sum: the client's update as the fp32 receipt f of rank r, kept as it is until the reducing
        call.  pinned: a view of a PinnedBuffer the caller keeps unchanged until the round is reduced."""
        f = np.ascontiguousarray(f)
        if f.dtype != np.float32:
            raise ValueError("need f float32")
        check(lib().fa_submit_lowrank_sum(self.handle, part, slot, f.ctypes.data, f.size, int(r), float(weight),
                                          HOST_PINNED if pinned else 0))

    def set_rot1_sum(self, on=True, part_id=-1):
        """fa_set_rot1_sum: the part's rounds take rot1 receipts (submit_rot1_sum) and reduce them in the rotated domain
        without expanding them, one transform per block and seed; on=False removes the stage."""
        check(lib().fa_set_rot1_sum(self.handle, part_id, 1 if on else 0))

    def submit_rot1_sum(self, part, slot, bits, scale, seed, weight=1.0, pinned=False):
        """fa_submit_rot1_sum: the client's update as (bits uint32[128 nb], scale float32[nb], seed), kept as it is until
        the reducing call.  pinned: views of PinnedBuffers the caller keeps unchanged until the round is reduced."""
        bits, scale = np.ascontiguousarray(bits), np.ascontiguousarray(scale)
        if bits.dtype != np.uint32 or scale.dtype != np.float32:
            raise ValueError("need bits uint32 and scale float32")
        if part in self.parts:
            nb = rot1_blocks(self.parts[part][0])
            if bits.size != nb * 128 or scale.size != nb:
                raise ValueError("bucket %d expects %d words and %d scales, got %d and %d"
                                 % (part, nb * 128, nb, bits.size, scale.size))
        check(lib().fa_submit_rot1_sum(self.handle, part, slot, bits.ctypes.data, scale.ctypes.data, int(seed), float(weight),
                                       HOST_PINNED if pinned else 0))

    def set_rot1(self, on=True, part=None):
        """fa_set_rot1: the part takes rot1 receipts, on the stage and the reference of set_mx8 (part None: the default
        of parts defined later); on=False switches them off."""
        check(lib().fa_set_rot1(self.handle, -1 if part is None else part, 1 if on else 0))

    def submit_rot1(self, part, slot, bits, scale, seed, weight=1.0, absolute=False, pinned=False):
        """fa_submit_rot1: the client's update against the part's last output as (bits uint32[128 nb], scale
        float32[nb], seed), expanded into the slot on the GPU.  pinned: views of PinnedBuffers the caller keeps
        unchanged until finalize returns.  absolute: the values themselves, no reference."""
        bits, scale = np.ascontiguousarray(bits), np.ascontiguousarray(scale)
        if bits.dtype != np.uint32 or scale.dtype != np.float32:
            raise ValueError("need bits uint32 and scale float32")
        if part in self.parts:
            nb = rot1_blocks(self.parts[part][0])
            if bits.size != nb * 128 or scale.size != nb:
                raise ValueError("bucket %d expects %d words and %d scales, got %d and %d"
                                 % (part, nb * 128, nb, bits.size, scale.size))
        flags = (HOST_PINNED if pinned else 0) | (ROT1_ABSOLUTE if absolute else 0)
        check(lib().fa_submit_rot1(self.handle, part, slot, bits.ctypes.data, scale.ctypes.data, int(seed), float(weight), flags))

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
