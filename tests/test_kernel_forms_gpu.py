"""GPU: every kernel form, on guard-banded buffers that carry IEEE edge values.

Each case (1) asserts the form it takes -- fa.plan_chain on the device's CU count for the chain forms, the
alignment rule of reduce_on / sync_on (vector form only where every pointer shares one 16-byte phase) for the
scalar ones -- and prints it; (2) builds its inputs, output, init and state in GuardedBufs (tests/guarded.py);
(3) runs the entry once; (4) checks, each reported on its own line of the failure: the whole result against the
oracle's fp32 chain (NaN-aware, bit-exact), the guards of every buffer the call may write, and the bits and
guards of every buffer it may only read.  The reference of every case is proven to hold its classes (NaN, both
infinities, both zeros, kept subnormals, overflow, the named rounding ties) before the GPU is touched.

Shapes follow from the CU count (fa.plan_chain(..., cus=)), never from 256; a case whose form this device
does not take skips with the reason.
"""
import ctypes

import numpy as np
import pytest

import guarded as G
from guarded import BF16, F16, F32, GuardedBuf

pytestmark = pytest.mark.gpu

def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


class Checks:
    """Collects the failures of one case, so parity, guards and read-only buffers are reported separately."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def run(self, what, fn, *a):
        try:
            fn(*a)
        except AssertionError as e:
            self.bad.append("[%s] %s" % (what, e))

    def done(self):
        assert not self.bad, "%s:\n" % self.case + "\n".join(self.bad)


class tuned:
    """fa.set_tuning for the block, the process tuning restored on the way out."""

    def __init__(self, fa, **kw):
        self.fa, self.kw = fa, kw

    def __enter__(self):
        self.before = self.fa.get_tuning()
        if self.kw:
            self.fa.set_tuning(**self.kw)

    def __exit__(self, *exc):
        restore = dict(self.before)
        restore["max_blocks"] = restore["max_blocks"] or -1
        restore["slot_skew"] = restore["slot_skew"] or -1
        self.fa.set_tuning(**restore)


def split_of(ptrs, n, dt, out_ptr=None, out_dt=None, init_ptr=None, literal=False):
    """(head, nvec, vector form?) of reduce_on / sync_on for these addresses: the vector form needs every
    input on one 16-byte phase, and the output (and init) aligned once the head elements are done."""
    si, V = G.ITEM[dt], G.vec_elems(dt)
    phase = (ptrs[-1 if literal else 0] % 16) // si
    head = min((V - phase) % V, n)
    vec = literal or all((p % 16) // si == phase for p in ptrs)
    if out_ptr is not None:
        so = G.ITEM[out_dt]
        vec = vec and (out_ptr + head * so) % min(16, V * so) == 0
    if init_ptr is not None:
        vec = vec and (init_ptr + head * 4) % 16 == 0
    return head, (n - head) // V, vec


def expect_form(fa, torch, case, in_dt, out_dt, n_body, D, want):
    """want: ("one-shot",), ("scalar",) or ("phased", phases or None).  The plan under the process tuning."""
    kind, nph = fa.plan_chain(G.fa_dt(fa, in_dt), G.fa_dt(fa, out_dt), n_body, D, cus=cus(torch))
    got = {fa.PLAN_ONE_SHOT: ("one-shot",), fa.PLAN_SCALAR: ("scalar",), fa.PLAN_PHASED: ("phased", nph)}[kind]
    ok = got[0] == want[0] and (len(want) < 2 or want[1] is None or want[1] == got[1])
    if not ok:
        msg = "%s: a device of %d CUs plans %s, the case needs %s" % (case, cus(torch), got, want)
        assert cus(torch) < 256, msg  # a whole chip takes every form
        pytest.skip(msg)
    return got


def chain_case(fa, O, torch, case, in_dt, out_dt, n, D, want, offs=None, out_off=None, init=None, seams=(),
               ctx=False, tuning=None, mode="fedavg"):
    """One chain (or literal) launch through fa.reduce_device; see the module docstring.  offs[k] / out_off: the
    16-byte phase in bytes of client k / the output; init: None, "separate" or "in place"."""
    import time
    t0 = time.time()
    offs = list(offs) if offs is not None else [0] * D
    with tuned(fa, **(tuning or {})):
        e = G.edge_inputs(O, n, D, in_dt, out_dt, seams=seams, with_init=init is not None)
        if mode == "literal":
            ref = G.literal_reference(O, e.xs[-1], in_dt, out_dt)
        else:
            ref, r32 = G.reference(O, e.xs, in_dt, e.w, out_dt, init=e.init)
            if n >= 4096:  # a smaller bucket holds the first rows of the table only
                G.classes_present(e, ref, r32)
        bufs, views = G.to_device(torch, fa, e, offs)
        ibuf = iview = None
        if init is not None:
            ibuf, iview = G.init_to_device(torch, fa, e, (out_off or 0) if init == "in place" else offs[0] * 4 // G.ITEM[in_dt])
        if init == "in place":
            assert out_dt == F32
            obuf = ibuf
        else:
            obuf = GuardedBuf(torch, n * G.ITEM[out_dt], offs[0] * G.ITEM[out_dt] // G.ITEM[in_dt] if out_off is None else out_off)
        oview = obuf.view(G.torch_bits_dtype(torch, out_dt))
        head, nvec, vec = split_of([b.ptr for b in bufs], n, in_dt, obuf.ptr, out_dt, ibuf.ptr if ibuf else None,
                                   literal=mode == "literal")
        if want[0] == "by the pointers":
            want = ("one-shot",) if vec else ("scalar",)
        if want[0] == "scalar" or mode == "literal":
            assert vec == (want[0] != "scalar"), "%s: the pointers give the %s form" % (case, "vector" if vec else "scalar")
            form = want
        else:
            assert vec, "%s: the pointers do not allow the vector form" % case
            form = expect_form(fa, torch, case, in_dt, out_dt, n - head, min(D, 128), want)
        snaps = [G.snapshot(v) for v in views]
        isnap = G.snapshot(iview) if ibuf is not None and init == "separate" else None
        agg = fa.Aggregator(1) if ctx else None
        try:
            fa.reduce_device([b.ptr for b in bufs], e.w if mode != "literal" else np.zeros(D, np.float32), n,
                             G.fa_dt(fa, in_dt), obuf.ptr, G.fa_dt(fa, out_dt),
                             fa.LITERAL if mode == "literal" else fa.FEDAVG, init=ibuf.ptr if ibuf else None, ctx=agg)
            if agg:
                agg.sync()
            torch.cuda.synchronize()
            c = Checks(case)
            c.run("parity", G.assert_bits_nan_aware, G.device_bits(oview, out_dt), ref, out_dt, "output")
            c.run("output guards", obuf.check, "output")
            for k, (b, v, s) in enumerate(zip(bufs, views, snaps)):
                c.run("client %d guards" % k, b.check, "client %d" % k)
                c.run("client %d read-only" % k, G.assert_unchanged, v, s, "client %d" % k)
            if isnap is not None:
                c.run("init guards", ibuf.check, "init")
                c.run("init read-only", G.assert_unchanged, iview, isnap, "init")
        finally:
            if agg:
                agg.close()
    print("form %s: %s, n = %d, D = %d, head %d, %.2f s" % (case, form, n, D, head, time.time() - t0))
    c.done()


def phase_elems(fa, torch, in_dt, out_dt, D=3):
    """Elements of one full phase under the process tuning: the smallest bucket of D < 16 clients the plan
    calls phased, and the elements one phase holds."""
    i, o = G.fa_dt(fa, in_dt), G.fa_dt(fa, out_dt)

    def first(pred):
        lo, hi = 1, 1 << 31
        if not pred(hi):
            return None
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
        return lo

    one = first(lambda n: fa.plan_chain(i, o, n, D, cus=cus(torch))[0] == fa.PLAN_PHASED)
    if one is None:
        pytest.skip("this device takes no phased plan for %s -> %s" % (in_dt, out_dt))
    # the smallest bucket may already take two phases (the odd XCDs leave LDS rows to the even ones, so a phase
    # holds less than the grid could): the step from two phases to three gives the phase
    V = G.vec_elems(in_dt)
    three = first(lambda n: fa.plan_chain(i, o, n, D, cus=cus(torch))[1] >= 3)
    return one, (three // V - 1) // 2 * V  # (smallest phased bucket, elements per phase)


# ------------------------------------------------------------------ one-shot chain

@pytest.mark.parametrize("in_dt,out_dt", G.PAIRS)
def test_one_shot_linear_every_head_and_tail(fa, O, torch_gpu, in_dt, out_dt):
    """n in {1, V-1, V, V+1, 4099} on every head 0..V-1 (the clients' 16-byte phase); on the phases 0, 1 and
    V-1 also every tail 0..V-1 after a body of whole vectors."""
    V = G.vec_elems(in_dt)
    for ph in range(V):
        sizes = {1, V - 1, V, V + 1, 4099}
        if ph in (0, 1, V - 1):
            sizes |= {4096 + ph + t for t in range(V)}
        for n in sorted(sizes):
            # a bucket that ends inside the head: vector form (head elements only) or scalar, by where the
            # output lands after them -- split_of applies reduce_on's rule to the addresses
            want = ("by the pointers",) if n < (V - ph) % V else ("one-shot",)
            chain_case(fa, O, torch_gpu, "one-shot %s->%s phase %d n %d" % (in_dt, out_dt, ph, n), in_dt, out_dt, n, 3,
                       want, offs=[ph * G.ITEM[in_dt]] * 3)


@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (F32, F16)])
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("walk", [2, 3])
def test_one_shot_xcd_walks(fa, O, torch_gpu, walk, block, in_dt, out_dt):
    n = 8 * block * G.vec_elems(in_dt) + 7
    chain_case(fa, O, torch_gpu, "xcd walk %d block %d %s->%s" % (walk, block, in_dt, out_dt), in_dt, out_dt, n, 3,
               ("one-shot",), tuning=dict(walk=walk, block=block, max_blocks=-1), seams=[j * (n // 8) for j in range(1, 8)])


@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (F16, F32)])
@pytest.mark.parametrize("max_blocks", [1, 7])
def test_capped_grid_stride(fa, O, torch_gpu, max_blocks, in_dt, out_dt):
    chain_case(fa, O, torch_gpu, "capped grid %d %s->%s" % (max_blocks, in_dt, out_dt), in_dt, out_dt, 100_003, 3,
               ("one-shot",), tuning=dict(max_blocks=max_blocks, walk=1), seams=(256 * 4 * max_blocks,))


@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (F32, BF16), (F16, F16)])  # st16, st8 and st16 of packed halves
@pytest.mark.parametrize("load_policy", [1, 2])
@pytest.mark.parametrize("store_policy", [1, 2, 3, 4])
def test_store_and_load_policies(fa, O, torch_gpu, store_policy, load_policy, in_dt, out_dt):
    chain_case(fa, O, torch_gpu, "store %d load %d %s->%s" % (store_policy, load_policy, in_dt, out_dt), in_dt, out_dt,
               16_391, 3, ("one-shot",), tuning=dict(store_policy=store_policy, load_policy=load_policy, walk=1))


@pytest.mark.parametrize("in_dt,out_dt", G.PAIRS)
@pytest.mark.parametrize("how", ["mixed phases", "output off phase"])
def test_scalar_plan(fa, O, torch_gpu, how, in_dt, out_dt):
    si = G.ITEM[in_dt]
    offs = [0, si, 3 * si] if how == "mixed phases" else [0, 0, 0]
    out_off = 0 if how == "mixed phases" else G.ITEM[out_dt]
    chain_case(fa, O, torch_gpu, "scalar, %s, %s->%s" % (how, in_dt, out_dt), in_dt, out_dt, 4099, 3, ("scalar",),
               offs=offs, out_off=out_off)


@pytest.mark.parametrize("in_dt", [F32, BF16, F16])
@pytest.mark.parametrize("init", ["separate", "in place"])
def test_init_chain(fa, O, torch_gpu, init, in_dt):
    for ph in (0, 1):
        chain_case(fa, O, torch_gpu, "init %s, %s->f32 phase %d" % (init, in_dt, ph), in_dt, F32, 4099, 3,
                   ("one-shot",), offs=[ph * G.ITEM[in_dt]] * 3, out_off=ph * 4, init=init)


@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (F16, F16)])
def test_two_passes_over_130_clients(fa, O, torch_gpu, in_dt, out_dt):
    """D = 130: 128 clients into an fp32 accumulator (the output itself, or ctx scratch for a 16-bit output),
    then the INIT continuation over the last 2."""
    chain_case(fa, O, torch_gpu, "two passes %s->%s" % (in_dt, out_dt), in_dt, out_dt, 50_003, 130, ("one-shot",),
               ctx=out_dt != F32)


# ------------------------------------------------------------------ phased chain

def sized_lanes(torch, in_dt):
    return cus(torch) * (256 if in_dt == F32 else 512)  # walk 5: the 256-thread f32 form, 512 threads for 16-bit inputs


@pytest.mark.parametrize("in_dt,out_dt", G.PAIRS)
def test_phased_sized_lds_only(fa, O, torch_gpu, in_dt, out_dt):
    """walk 5, D = 16, the smallest accepted q: every vector of the one sized phase goes through LDS -- fp32
    rows for an fp32 output, packed 16-bit rows for a 16-bit one."""
    V = G.vec_elems(in_dt)
    q = 8 if in_dt == F32 else 4
    n = q * sized_lanes(torch_gpu, in_dt) * V - 5
    chain_case(fa, O, torch_gpu, "phased sized LDS only %s->%s q %d" % (in_dt, out_dt, q), in_dt, out_dt, n, 16,
               ("phased", 1), tuning=dict(walk=5), seams=[j * (n // q) for j in range(1, q)])


@pytest.mark.parametrize("q,init", [(40 + 8, None), (40 + 16, "in place")])
def test_phased_sized_registers_and_lds(fa, O, torch_gpu, q, init):
    """q = RL + 8 vectors per lane (RL = 160 KiB / (256 * 16 B) = 40: all 48 in the register stage) and RL + 16
    (48 in registers, 8 in LDS; the INIT continuation in place), each minus half a row, so the last wave chunk
    crosses the end of the bucket (stage_regs gives up, the lane stores its own)."""
    lanes = sized_lanes(torch_gpu, F32)
    n = q * lanes * 4 - lanes * 2
    chain_case(fa, O, torch_gpu, "phased sized q %d%s" % (q, ", init in place" if init else ""), F32, F32, n, 16,
               ("phased", 1), tuning=dict(walk=5), init=init, seams=[j * lanes * 4 for j in (8, 40, q - 1)])


@pytest.mark.parametrize("walk,shape", [(5, "smallest"), (5, "x1.05"), (5, "+12345"), (5, "+offset 1"),
                                        (4, "+offset 1"), (6, "+offset 1")])
def test_phased_full_and_balanced_last_phase(fa, O, torch_gpu, walk, shape):
    torch = torch_gpu
    with tuned(fa, walk=walk):
        one, per = phase_elems(fa, torch, F32, F32)
    n, ph = {"smallest": (one, 0), "x1.05": (int(one * 1.05), 0), "+12345": (one + 12_345, 0),
             "+offset 1": (one + 12_345 + 4, 1)}[shape]
    chain_case(fa, O, torch, "phased walk %d %s" % (walk, shape), F32, F32, n, 3, ("phased", None), tuning=dict(walk=walk),
               offs=[4 * ph] * 3, seams=[per, per + (4 - ph) % 4, n - 12_345])


@pytest.mark.parametrize("in_dt,out_dt", [(BF16, BF16), (F16, F16), (F32, BF16), (F16, F32)])
def test_phased_full_row_types(fa, O, torch_gpu, in_dt, out_dt):
    """One full phase and a balanced second one per LDS row type beyond f32 -> f32 (above): packed 16-bit rows
    from 16-bit and from fp32 inputs, fp32 rows from 16-bit inputs."""
    torch = torch_gpu
    with tuned(fa, walk=5):
        one, per = phase_elems(fa, torch, in_dt, out_dt)
    n = one + 12_345
    chain_case(fa, O, torch, "phased full %s->%s" % (in_dt, out_dt), in_dt, out_dt, n, 3, ("phased", 2),
               tuning=dict(walk=5), seams=[per])


# ------------------------------------------------------------------ literal

@pytest.mark.parametrize("in_dt,out_dt", G.PAIRS)
@pytest.mark.parametrize("how", ["aligned", "same phase 1", "output off phase"])
def test_literal_vec_and_scalar(fa, O, torch_gpu, how, in_dt, out_dt):
    si, so = G.ITEM[in_dt], G.ITEM[out_dt]
    offs, out_off = {"aligned": ([0] * 3, 0), "same phase 1": ([si] * 3, so), "output off phase": ([0] * 3, so)}[how]
    chain_case(fa, O, torch_gpu, "literal %s %s->%s" % (how, in_dt, out_dt), in_dt, out_dt, 4099, 3,
               ("scalar",) if how == "output off phase" else ("vector",), offs=offs, out_off=out_off, mode="literal")


# ------------------------------------------------------------------ state sync

def sync_case(fa, O, torch, case, dt, n, D, form, offs=None, ctx=False, tuning=None, seams=()):
    import time
    t0 = time.time()
    offs = list(offs) if offs is not None else [0] * D
    with tuned(fa, **(tuning or {})):
        e = G.edge_inputs(O, n, D, dt, dt, seams=seams)
        ref, r32 = G.reference(O, e.xs, dt, e.w, dt)
        G.classes_present(e, ref, r32)
        bufs, views = G.to_device(torch, fa, e, offs)
        head, nvec, vec = split_of([b.ptr for b in bufs], n, dt)
        if form == "scalar":
            assert not vec
        elif form != "broadcast":
            assert vec
        if form == "phased":  # launch_sync_phased_r: at least one whole phase of the dt -> dt register form
            lanes_vecs = cus(torch) * 256 * (160 * 1024 // (256 * 16) + 192 // G.vec_elems(dt))
            if cus(torch) < 256:
                pytest.skip("%s: shape sized for a whole chip, this device has %d CUs" % (case, cus(torch)))
            assert nvec >= lanes_vecs and fa.plan_chain(G.fa_dt(fa, dt), G.fa_dt(fa, dt), n, D, cus=cus(torch))[0] == fa.PLAN_PHASED
        elif form == "vector":
            assert fa.plan_chain(G.fa_dt(fa, dt), G.fa_dt(fa, dt), n, D, cus=cus(torch))[0] == fa.PLAN_ONE_SHOT
        agg = fa.Aggregator(1) if ctx else None
        try:
            fa.sync_device([b.ptr for b in bufs], e.w, n, G.fa_dt(fa, dt), ctx=agg)
            if agg:
                agg.sync()
            torch.cuda.synchronize()
            c = Checks(case)
            for k, (b, v) in enumerate(zip(bufs, views)):
                c.run("slot %d parity" % k, G.assert_bits_nan_aware, G.device_bits(v, dt), ref, dt, "slot %d" % k)
                c.run("slot %d guards" % k, b.check, "slot %d" % k)
        finally:
            if agg:
                agg.close()
    print("form %s: sync %s, n = %d, D = %d, head %d, %.2f s" % (case, form, n, D, head, time.time() - t0))
    c.done()


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("form", ["vector", "vector, phase 1", "scalar", "broadcast"])
def test_sync_forms(fa, O, torch_gpu, form, dt):
    si = G.ITEM[dt]
    if form == "broadcast":
        sync_case(fa, O, torch_gpu, "sync broadcast %s" % dt, dt, 4099, 130, "broadcast", ctx=True)
    elif form == "scalar":
        sync_case(fa, O, torch_gpu, "sync scalar %s" % dt, dt, 4099, 3, "scalar", offs=[0, si, 3 * si])
    else:
        ph = 1 if "phase 1" in form else 0
        sync_case(fa, O, torch_gpu, "sync %s %s" % (form, dt), dt, 4099, 3, "vector", offs=[ph * si] * 3)


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_sync_phased_one_full_phase(fa, O, torch_gpu, dt):
    torch = torch_gpu
    V = G.vec_elems(dt)
    per = cus(torch) * 256 * (40 + 192 // V) * V  # walk 5's sync form: RL 40 + RR 48 (f32) / 24 (16-bit) vectors per lane
    sync_case(fa, O, torch, "sync phased %s" % dt, dt, per + 12_345, 3, "phased", tuning=dict(walk=5), seams=[per])


# ------------------------------------------------------------------ segment table (fa_reduce_parts)

def _hip():
    return ctypes.CDLL("libamdhip64.so.7")  # the runtime torch already loaded


def _memcpy(hip, dst, src, nbytes, kind):
    fn = hip.hipMemcpy
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert fn(dst, src, nbytes, kind) == 0


@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (F32, F16)])
@pytest.mark.parametrize("max_d", [8, 9])
def test_segment_table_three_parts(fa, O, torch_gpu, max_d, in_dt, out_dt):
    """Three small FedAvg parts in one batched launch: parity on edge values, every slot (read back through
    its agg.slot pointer) keeps its bits, and each part's output is its own -- the same parts reduced with
    their neighbours' data replaced give the same bits."""
    torch = torch_gpu
    hip = _hip()
    sizes = {2: (1, 3), 3: (4099, max_d), 4: (65_537, 5)}
    case = "segment table max_d %d %s->%s" % (max_d, in_dt, out_dt)
    c = Checks(case)
    with fa.Aggregator(1) as agg:
        data = {}
        for pid, (n, D) in sizes.items():
            agg.define(pid, n, G.fa_dt(fa, in_dt), G.fa_dt(fa, out_dt), D)
            e = G.edge_inputs(O, n, D, in_dt, out_dt, seed=0x5EED + pid)
            ref, r32 = G.reference(O, e.xs, in_dt, e.w, out_dt)
            if n >= 4096:
                G.classes_present(e, ref, r32)
            for k in range(D):
                ptr, cnt, off = agg.slot(pid, 0, k)
                assert (cnt, off) == (n, 0)
                _memcpy(hip, ptr, e.xs[k].ctypes.data, e.xs[k].nbytes, 1)
            data[pid] = (e, ref)
        ws = [data[pid][0].w for pid in sizes]
        agg.reduce_parts(list(sizes), ws)
        agg.sync()
        outs = {}
        for pid, (n, D) in sizes.items():
            e, ref = data[pid]
            outs[pid] = agg.copy_output(pid).view(G.BITS[out_dt])
            c.run("part %d parity" % pid, G.assert_bits_nan_aware, outs[pid], ref, out_dt, "part %d" % pid)
            for k in range(D):
                back = np.empty_like(e.xs[k])
                _memcpy(hip, back.ctypes.data, agg.slot(pid, 0, k)[0], back.nbytes, 2)
                c.run("part %d slot %d read-only" % (pid, k), lambda a, b: np.testing.assert_array_equal(a, b), back, e.xs[k])
    # neighbours replaced: part 3 keeps its bits whatever parts 2 and 4 hold
    with fa.Aggregator(1) as agg:
        for pid, (n, D) in sizes.items():
            agg.define(pid, n, G.fa_dt(fa, in_dt), G.fa_dt(fa, out_dt), D)
            for k in range(D):
                ptr = agg.slot(pid, 0, k)[0]
                if pid == 3:
                    _memcpy(hip, ptr, data[3][0].xs[k].ctypes.data, data[3][0].xs[k].nbytes, 1)
                else:
                    fa.fill_uniform(ptr, n, G.fa_dt(fa, in_dt), 77, k)
        agg.reduce_parts(list(sizes), ws)
        agg.sync()
        c.run("part 3 unaffected by its neighbours", G.assert_bits_nan_aware, agg.copy_output(3).view(G.BITS[out_dt]),
              outs[3], out_dt, "part 3")
    print("form %s: segment table (fa_reduce_parts, one launch)" % case)
    c.done()


# ------------------------------------------------------------------ stages: guards and read-only inputs

def _guarded_clients(fa, torch, n, D, dt, offs):
    bufs = []
    for k in range(D):
        b = GuardedBuf(torch, n * G.ITEM[dt], offs[k % len(offs)])
        fa.fill_uniform(b.ptr, n, G.fa_dt(fa, dt), 0x7A1, k)
        bufs.append(b)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (F16, F32)])
@pytest.mark.parametrize("how", ["aligned", "phase 1", "output off phase"])
@pytest.mark.parametrize("D", [3, 8, 65, 128])
def test_trimmed_forms_write_only_their_output(fa, torch_gpu, D, how, in_dt, out_dt):
    """The trimmed vector, element and wide (D > 64) kernels: guards of the output, guards and bits of every
    client (the values are covered by tests/test_trimmed_gpu.py)."""
    torch = torch_gpu
    n, si, so = 4099, G.ITEM[in_dt], G.ITEM[out_dt]
    offs, out_off = {"aligned": ([0], 0), "phase 1": ([si], so), "output off phase": ([0], so)}[how]
    bufs = _guarded_clients(fa, torch, n, D, in_dt, offs)
    views = [b.view(G.torch_bits_dtype(torch, in_dt)) for b in bufs]
    snaps = [G.snapshot(v) for v in views]
    obuf = GuardedBuf(torch, n * so, out_off)
    oview = obuf.view(G.torch_bits_dtype(torch, out_dt))
    before = G.snapshot(oview)
    fa.trimmed_device([b.ptr for b in bufs], n, G.fa_dt(fa, in_dt), obuf.ptr, G.fa_dt(fa, out_dt), trim=1)
    torch.cuda.synchronize()
    case = "trimmed D %d %s %s->%s" % (D, how, in_dt, out_dt)
    c = Checks(case)
    c.run("output guards", obuf.check, "output")
    # uniform inputs in [-1, 1): every written element differs from the pre-fill pattern somewhere
    c.run("output written", lambda: _assert(int((oview != before).sum()) > n * 0.9, "most of the output still holds the pre-fill"))
    for k, (b, v, s) in enumerate(zip(bufs, views, snaps)):
        c.run("client %d guards" % k, b.check, "client %d" % k)
        c.run("client %d read-only" % k, G.assert_unchanged, v, s, "client %d" % k)
    print("form %s: trimmed %s" % (case, "wide" if D > 64 else "vector + element edges" if how != "output off phase" else "element"))
    c.done()


def _assert(cond, msg):
    assert cond, msg


@pytest.mark.parametrize("how", ["vector, out", "vector, states only", "vector, out is avg", "element, phase mix",
                                 "vector, bf16 out", "element, f16 out off phase"])
@pytest.mark.parametrize("rule", ["momentum", "adagrad", "adam", "yogi"])
def test_server_opt_forms_write_only_their_arrays(fa, torch_gpu, rule, how):
    torch = torch_gpu
    n = 4099
    rule_id = {"momentum": fa.OPT_MOMENTUM, "adagrad": fa.OPT_ADAGRAD, "adam": fa.OPT_ADAM, "yogi": fa.OPT_YOGI}[rule]
    ph = [4, 4, 4, 4] if how.startswith("vector") else [0, 4, 8, 12]
    avg, x, m, v = [GuardedBuf(torch, n * 4, p) for p in ph]
    for j, b in enumerate((avg, x, m, v)):
        fa.fill_uniform(b.ptr, n, fa.F32, 0x0B7, j)
    v.view(torch.float32).abs_()  # a second moment is not negative
    if rule == "momentum":
        v_arg = None  # d_v NULL: the rule has no second moment, the buffer must stay as it is
    else:
        v_arg = v.ptr
    out_dt = BF16 if "bf16" in how else F16 if "f16" in how else F32
    out = None
    if "states only" in how:
        out_arg = None
    elif "out is avg" in how:
        out_arg = avg.ptr
    else:
        out = GuardedBuf(torch, n * G.ITEM[out_dt], (ph[0] * G.ITEM[out_dt] // 4) if "off phase" not in how else 2)
        out_arg = out.ptr
    torch.cuda.synchronize()
    avg_view = avg.view(torch.int32)
    snap_avg, snap_v = G.snapshot(avg_view), G.snapshot(v.view(torch.int32))
    fa.server_opt_device(avg.ptr, x.ptr, m.ptr, v_arg, n, out_arg, G.fa_dt(fa, out_dt), rule=rule_id, lr=0.5, beta1=0.9,
                         beta2=0.99, tau=1e-3)
    torch.cuda.synchronize()
    case = "server opt %s, %s" % (rule, how)
    c = Checks(case)
    for name, b in (("avg", avg), ("x", x), ("m", m), ("v", v)) + ((("out", out),) if out is not None else ()):
        c.run("%s guards" % name, b.check, name)
    if "out is avg" not in how:
        c.run("avg read-only", G.assert_unchanged, avg_view, snap_avg, "avg")
    if rule == "momentum":
        c.run("v untouched", G.assert_unchanged, v.view(torch.int32), snap_v, "v")
    print("form %s" % case)
    c.done()


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("how", ["vector", "vector, phase 1", "element"])
@pytest.mark.parametrize("D", [3, 130])
def test_clip_sumsq_reads_only(fa, torch_gpu, D, how, dt):
    torch = torch_gpu
    n, si = 4099, G.ITEM[dt]
    offs = [0] if how == "vector" else [si] if how == "vector, phase 1" else [0, si, 3 * si]
    bufs = _guarded_clients(fa, torch, n, D, dt, offs)
    views = [b.view(G.torch_bits_dtype(torch, dt)) for b in bufs]
    ref = GuardedBuf(torch, n * 4, 4 if how == "vector, phase 1" else 0)
    fa.fill_uniform(ref.ptr, n, fa.F32, 0x7A1, 999)
    torch.cuda.synchronize()
    rview = ref.view(torch.int32)
    snaps, rsnap = [G.snapshot(v) for v in views], G.snapshot(rview)
    q = fa.clip_sumsq_device([b.ptr for b in bufs], n, G.fa_dt(fa, dt), ref.ptr)
    torch.cuda.synchronize()
    case = "clip sumsq D %d %s %s" % (D, how, dt)
    c = Checks(case)
    c.run("sums", lambda: _assert(bool(np.isfinite(q).all() and (q > 0).all()), "Q = %r" % (q,)))  # values: test_clip_gpu.py
    c.run("reference guards", ref.check, "reference")
    c.run("reference read-only", G.assert_unchanged, rview, rsnap, "reference")
    for k, (b, v, s) in enumerate(zip(bufs, views, snaps)):
        c.run("client %d guards" % k, b.check, "client %d" % k)
        c.run("client %d read-only" % k, G.assert_unchanged, v, s, "client %d" % k)
    print("form %s" % case)
    c.done()


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("n", [1, 7, 4099])
def test_fill_writes_only_its_elements(fa, O, torch_gpu, n, dt):
    torch = torch_gpu
    c = Checks("fill %s n %d" % (dt, n))
    for off in range(0, 16, G.ITEM[dt]):
        b = GuardedBuf(torch, n * G.ITEM[dt], off)
        fa.fill_uniform(b.ptr, n, G.fa_dt(fa, dt), 0x5EED, 5, 17)
        torch.cuda.synchronize()
        want = O.gen(0x5EED, 5, n, idx0=17, dtype="bf16") if dt == BF16 else O.gen(0x5EED, 5, n, idx0=17).view(np.uint32)
        c.run("values at +%d" % off, G.assert_bits_nan_aware, G.device_bits(b.view(G.torch_bits_dtype(torch, dt)), dt), want, dt, "fill")
        c.run("guards at +%d" % off, b.check, "fill at +%d" % off)
    print("form fill %s n %d: every 16-byte phase" % (dt, n))
    c.done()
