"""Guard-band buffers and IEEE edge-value datasets for the kernel tests.

Two things the parity tests could not see before:

* where a kernel writes -- ``GuardedBuf`` puts 64 KiB of a position-dependent byte pattern before and after
  the payload (inside one allocation, so a stray store faults nothing) and ``check()`` proves it is still there;
  ``snapshot`` / ``assert_unchanged`` do the same for the payload of a buffer a call may only read;
* what a kernel form does with IEEE edge values -- ``edge_inputs`` starts from the oracle generator's uniform
  data (the bytes fa_fill_uniform writes) and overwrites chosen positions with rows of ``edge_table``: signed
  zeros, infinities, NaN, subnormals, the largest finite value, sums that overflow or cancel into the
  subnormal range, and exact rounding ties of a 16-bit output.  ``to_device`` builds the same bytes on the
  device with a fill and one index_put, so multi-million-element shapes cost no full upload.

Everything here but ``to_device`` / ``GuardedBuf(torch, ...)`` runs without a GPU (tests/test_guarded_cpu.py).
The chain weights are powers of two (1, 1/2, 2^-20 ..., and 2^-130 for the last client), so every product of
a table row is exact in fp32 and the expected bits of a named tie can be written down.
"""
import numpy as np

F32, BF16, F16 = "f32", "bf16", "f16"
ITEM = {F32: 4, BF16: 2, F16: 2}
BITS = {F32: np.uint32, BF16: np.uint16, F16: np.uint16}
# the dtype pairs the library reduces (in, out)
PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, F16)]

GUARD = 64 << 10  # bytes on each side: more than one wave's register chunk (48 rows of 1 KiB)


def fa_dt(fa, dt):
    return {F32: fa.F32, BF16: fa.BF16, F16: fa.F16}[dt]


def vec_elems(dt):
    """Elements of one 16-byte input vector."""
    return 16 // ITEM[dt]


# ------------------------------------------------------------------ guard bands

def pattern(lo, hi):
    """The guard byte at allocation offsets [lo, hi): never zero, and it changes with the position."""
    p = np.arange(lo, hi, dtype=np.int64) % 251
    return ((p * 131 + 89) % 251 + 1).astype(np.uint8)


_TILE = {}


def _prefill(torch, base):
    L = 251 * 4096  # a whole number of pattern periods
    tile = _TILE.get(base.device)
    if tile is None:
        tile = _TILE[base.device] = torch.from_numpy(pattern(0, L)).to(base.device)
    for s in range(0, base.numel(), L):
        m = min(L, base.numel() - s)
        base[s:s + m].copy_(tile[:m])


class GuardedBuf:
    """guard + payload + guard in one uint8 allocation, pre-filled with pattern(); the payload starts at
    `elem_offset_bytes` modulo 16.  `torch` None: a numpy stand-in for the device allocation (CPU tests)."""

    def __init__(self, torch, nbytes, elem_offset_bytes=0):
        self.torch, self.nbytes = torch, int(nbytes)
        total = 2 * GUARD + self.nbytes + 16
        if torch is None:
            self.base = np.empty(total, np.uint8)
            self.base[:] = pattern(0, total)
            addr = self.base.ctypes.data
        else:
            self.base = torch.empty(total, dtype=torch.uint8, device="cuda")
            _prefill(torch, self.base)
            addr = self.base.data_ptr()
        self.start = GUARD + (elem_offset_bytes - (addr + GUARD)) % 16
        self.ptr = addr + self.start
        assert self.ptr % 16 == elem_offset_bytes % 16

    def payload(self):
        return self.base[self.start:self.start + self.nbytes]

    def view(self, dtype):
        """The payload as a typed view (a torch or numpy dtype)."""
        return self.payload().view(dtype)

    def _host(self, lo, hi):
        part = self.base[lo:hi]
        return part if self.torch is None else part.cpu().numpy()

    def damage(self):
        """None, or (side, first, last): the first and last damaged byte of a guard, as offsets from the
        payload edge -- negative before the payload, 0 = the first byte after it."""
        end = self.start + self.nbytes
        for side, lo, hi, edge in (("before", 0, self.start, self.start), ("after", end, self.base.shape[0], end)):
            bad = np.flatnonzero(self._host(lo, hi) != pattern(lo, hi))
            if bad.size:
                return side, int(bad[0]) + lo - edge, int(bad[-1]) + lo - edge
        return None

    def check(self, what=""):
        d = self.damage()
        assert d is None, "%s: guard %s the payload damaged, bytes %+d .. %+d from the payload edge" % (
            what, d[0], d[1], d[2])


def snapshot(t):
    """The bits of a device tensor, to compare after a call that may only read it."""
    import torch
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).clone()


def assert_unchanged(t, snap, what=""):
    import torch
    if not torch.equal(t.view(snap.dtype), snap):
        bad = torch.nonzero(t.view(snap.dtype) != snap).flatten()
        raise AssertionError("%s: read-only buffer changed at %d elements, first %d, last %d" % (
            what, bad.numel(), int(bad[0]), int(bad[-1])))


# ------------------------------------------------------------------ bits

def nan_mask(bits, dt):
    if dt == F32:
        return (bits & 0x7FFFFFFF) > 0x7F800000
    return (bits & 0x7FFF) > (0x7F80 if dt == BF16 else 0x7C00)


def assert_bits_nan_aware(got, ref, dt, what=""):
    """got, ref: the bits (uint32 / uint16) of dtype `dt`.  NaN positions must match (no reference defines a
    payload); everything else is bit-exact, the sign of zero included."""
    assert got.dtype == ref.dtype == BITS[dt] and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    gn, rn = nan_mask(got, dt), nan_mask(ref, dt)
    bad = np.flatnonzero(gn != rn)
    assert bad.size == 0, "%s: NaN positions differ at %d elements, first %s: got %s ref %s" % (
        what, bad.size, bad[:4], [hex(int(v)) for v in got[bad[:4]]], [hex(int(v)) for v in ref[bad[:4]]])
    bad = np.flatnonzero((got != ref) & ~gn)
    assert bad.size == 0, "%s: %d/%d mismatches, first at %s (last %d): got %s ref %s" % (
        what, bad.size, got.size, bad[:4], bad[-1], [hex(int(v)) for v in got[bad[:4]]],
        [hex(int(v)) for v in ref[bad[:4]]])


def rne16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32).astype(np.float16)


def to_bits(O, vals, dt):
    """fp32 values -> the bits of dtype `dt` (round to nearest even; table values are chosen exact)."""
    v = np.ascontiguousarray(vals, np.float32)
    if dt == F32:
        return v.view(np.uint32).copy()
    return O.f32_to_bf16(v) if dt == BF16 else rne16(v).view(np.uint16)


def widen(bits, dt):
    """The bits of dtype `dt` as fp32 values (exact)."""
    if dt == F32:
        return bits.view(np.float32)
    if dt == BF16:
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def round_out(O, r32, dt):
    """The fp32 chain result rounded once to the output dtype, as bits."""
    if dt == F32:
        return np.ascontiguousarray(r32, np.float32).view(np.uint32)
    return O.f32_to_bf16(r32) if dt == BF16 else rne16(r32).view(np.uint16)


def chain_weights(D):
    """Powers of two: 1, 1/2, then 2^-20, and 2^-130 for the last client (its products underflow)."""
    assert D >= 3
    w = np.full(D, 2.0 ** -20, np.float32)
    w[0], w[1], w[-1] = 1.0, 0.5, 2.0 ** -130
    return w


def reference(O, xs, in_dt, w, out_dt, init=None):
    """(bits in out_dt, fp32 chain) of the ordered fp32 fma chain over the widened inputs: the oracle."""
    r32 = O.fedavg([np.ascontiguousarray(widen(x, in_dt)) for x in xs], w, init=init, threads=8)
    return round_out(O, r32, out_dt), r32


def literal_reference(O, x_last, in_dt, out_dt):
    return round_out(O, O.literal(np.ascontiguousarray(widen(x_last, in_dt))), out_dt)


# ------------------------------------------------------------------ edge values

_LIMITS = {  # smallest subnormal, largest subnormal, smallest normal, largest finite
    F32: (2.0 ** -149, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126, (2 - 2.0 ** -23) * 2.0 ** 127),
    BF16: (2.0 ** -133, 2.0 ** -126 - 2.0 ** -133, 2.0 ** -126, (2 - 2.0 ** -7) * 2.0 ** 127),
    F16: (2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 65504.0),
}
# named rounding ties of a 16-bit output: (name, x0, x1, bits) -- the chain value x0 + x1 / 2 is exact in fp32
_TIES = {
    F16: [("tie 1+ulp/2 -> even", 1.0, 2.0 ** -10, 0x3C00),
          ("tie 1+3ulp/2 -> even", 1.0 + 2.0 ** -10, 2.0 ** -10, 0x3C02),
          ("tie largest finite / inf -> inf", 65504.0, 32.0, 0x7C00),
          ("tie -largest finite / -inf -> -inf", -65504.0, -32.0, 0xFC00),
          ("tie half the smallest subnormal -> +0", 0.0, 2.0 ** -24, 0x0000),
          ("tie -half the smallest subnormal -> -0", 0.0, -2.0 ** -24, 0x8000),
          ("tie 1.5 subnormal steps -> even", 2.0 ** -24, 2.0 ** -24, 0x0002)],
    BF16: [("tie 1+ulp/2 -> even", 1.0, 2.0 ** -7, 0x3F80),
           ("tie 1+3ulp/2 -> even", 1.0 + 2.0 ** -7, 2.0 ** -7, 0x3F82),
           ("tie largest finite / inf -> inf", _LIMITS[BF16][3], 2.0 ** 120, 0x7F80),
           ("tie -largest finite / -inf -> -inf", -_LIMITS[BF16][3], -2.0 ** 120, 0xFF80),
           ("tie half the smallest subnormal -> +0", 0.0, 2.0 ** -133, 0x0000),
           ("tie -half the smallest subnormal -> -0", 0.0, -2.0 ** -133, 0x8000),
           ("tie 1.5 subnormal steps -> even", 2.0 ** -133, 2.0 ** -133, 0x0002)],
}


def edge_table(in_dt, out_dt):
    """Rows (name, x0, x1, x_last, bits): the values of clients 0, 1 and D-1 (the clients between hold +0) and,
    for a named tie, the output bits.  Every value is exact in `in_dt`."""
    m, M, N, X = _LIMITS[in_dt]
    inf, nan = np.inf, np.nan
    rows = [("zeros", 0.0, 0.0, 0.0), ("negative zeros", -0.0, -0.0, -0.0),
            ("underflow to -0", 0.0, 0.0, -m), ("underflow to +0", 0.0, 0.0, m),
            ("+inf", inf, 1.0, 1.0), ("-inf", 1.0, -inf, 1.0), ("inf - inf", inf, -inf, 0.0),
            ("nan", 1.0, nan, 0.0), ("nan first", nan, 1.0, 1.0), ("nan last", 0.0, 0.0, nan),
            ("inf last", 0.0, 0.0, inf), ("-inf first", -inf, 0.0, 0.0),
            ("smallest subnormal", m, 0.0, 0.0), ("-smallest subnormal", -m, 0.0, 0.0),
            ("largest subnormal", M, 0.0, 0.0), ("smallest normal", N, 0.0, 0.0),
            ("largest finite", X, 0.0, 0.0), ("-largest finite", -X, 0.0, 0.0),
            ("half the smallest subnormal", 0.0, m, 0.0), ("half the largest subnormal", 0.0, -M, 0.0),
            ("half the smallest normal", 0.0, N, 0.0), ("half the largest finite", 0.0, X, 0.0),
            ("sum overflows", X, X, 0.0), ("sum overflows down", -X, -X, 0.0),
            ("cancels into the subnormal range", 1.5 * N, -2.0 * N, 0.0),
            ("cancels into the subnormal range, negative", -1.25 * N, 2.0 * N, 0.0),
            ("cancels to zero", N, -2.0 * N, 0.0), ("subnormals add up to a normal", M, 2.0 * m, 0.0),
            ("last client lands in the fp32 subnormal range", 0.0, 0.0, 1.0),
            ("last client, negative", 0.0, 0.0, -1.5)]
    rows = [r + (None,) for r in rows]
    for name, x0, x1, bits in _TIES.get(out_dt, []):
        rows.append((name, x0, x1, 0.0, bits))
    return rows


_INIT_SPECIALS = np.array([-0.0, np.inf, -np.inf, np.nan, 2.0 ** -149, -_LIMITS[F32][3], 1.0, -2.0 ** -126], np.float32)


def positions(n, seams=(), seed=0):
    """Sorted element indices to cover: the first and last 4096, 64 either side of every seam (phase
    boundaries, head / body / tail), and a seeded random 1 % of the rest."""
    parts = [np.arange(0, min(n, 4096)), np.arange(max(0, n - 4096), n)]
    for e in seams:
        parts.append(np.arange(max(0, int(e) - 64), min(n, int(e) + 64)))
    rng = np.random.default_rng(seed)
    parts.append(rng.integers(0, n, n // 100))
    return np.unique(np.concatenate(parts)).astype(np.int64)


class EdgeData:
    """n, D, dtypes, weights, host inputs `xs` (bits), optional fp32 `init`, the covered positions `idx`
    and the table row `row[i]` planted at idx[i]."""


def edge_inputs(O, n, D, in_dt, out_dt, seams=(), seed=0x5EED, with_init=False):
    e = EdgeData()
    e.n, e.D, e.in_dt, e.out_dt, e.seed = n, D, in_dt, out_dt, seed
    e.w = chain_weights(D)
    e.table = edge_table(in_dt, out_dt)
    T = len(e.table)
    e.idx = positions(n, seams, seed)
    rank = np.arange(e.idx.size)
    e.row = rank % T
    cols = [to_bits(O, np.array([r[c] for r in e.table], np.float32), in_dt) for c in (1, 2, 3)]
    zero = to_bits(O, np.zeros(1, np.float32), in_dt)[0]
    e.vals = []  # per client: the bits planted at idx
    for k in range(D):
        e.vals.append(cols[0][e.row] if k == 0 else cols[1][e.row] if k == 1 else cols[2][e.row] if k == D - 1
                      else np.full(e.idx.size, zero, BITS[in_dt]))
    e.xs = []
    for k in range(D):
        x = O.gen(seed, k, n, dtype="bf16") if in_dt == BF16 else to_bits(O, O.gen(seed, k, n), in_dt)
        x[e.idx] = e.vals[k]
        e.xs.append(x)
    e.init = e.init_vals = None
    if with_init:
        # +0 on every other pass through the table, so that each row also appears as without an init
        cyc = rank // T
        e.init_vals = np.where(cyc % 2 == 0, np.float32(0.0), _INIT_SPECIALS[(cyc // 2 + e.row) % _INIT_SPECIALS.size])
        e.init_vals = e.init_vals.astype(np.float32)
        e.init = O.gen(seed, 999, n)
        e.init[e.idx] = e.init_vals
    return e


def check_table_exact(O, in_dt, out_dt):
    """Every table value survives the conversion to `in_dt` (so the device sees what the row says)."""
    for name, x0, x1, xl, _ in edge_table(in_dt, out_dt):
        for v in (x0, x1, xl):
            back = widen(to_bits(O, np.array([v], np.float32), in_dt), in_dt)[0]
            assert (np.isnan(v) and np.isnan(back)) or (back == v and np.signbit(back) == np.signbit(v)), (name, v, back)


def classes_present(e, ref_bits, r32):
    """The classes the reference of dataset `e` must contain, so no case is vacuous: returns {class: count}
    and asserts each reachable one is there and every named tie lands on its bits."""
    out_dt = e.out_dt
    top = BITS[out_dt](1) << (31 if out_dt == F32 else 15)
    mag = ref_bits & ~top
    inf_bits = {F32: 0x7F800000, BF16: 0x7F80, F16: 0x7C00}[out_dt]
    min_norm = {F32: 0x00800000, BF16: 0x0080, F16: 0x0400}[out_dt]
    finite32 = np.isfinite(r32)
    c = {"nan": int(nan_mask(ref_bits, out_dt).sum()),
         "+inf": int((ref_bits == inf_bits).sum()), "-inf": int((ref_bits == (inf_bits | top)).sum()),
         "+0": int((ref_bits == 0).sum()), "-0": int((ref_bits == top).sum()),
         "subnormal kept": int(((mag > 0) & (mag < min_norm)).sum()),
         # finite inputs (or a finite fp32 chain) whose result is infinite: the sum, or its rounding, overflowed
         "rounds to inf": int(((mag == inf_bits) & _finite_inputs(e)).sum())}
    for k, v in c.items():
        if k == "rounds to inf" and e.in_dt == F16 and out_dt == F32:
            continue  # fp16 inputs cannot overflow an fp32 chain with these weights
        assert v > 0, "the reference of %s -> %s holds no %s" % (e.in_dt, out_dt, k)
    if out_dt != F32:  # rounding of a finite fp32 chain value to inf
        assert int(((mag == inf_bits) & finite32).sum()) > 0
    ties = [(j, r) for j, r in enumerate(e.table) if r[4] is not None]
    assert len(ties) == len(_TIES.get(out_dt, []))
    for j, (name, x0, x1, xl, bits) in ties:
        at = np.flatnonzero(e.row == j)
        if e.init is not None:  # where the init is +0 the row is the tie it names
            at = at[e.init_vals.view(np.uint32)[at] == 0]
        assert at.size >= 2, name
        got = ref_bits[e.idx[at]]
        assert np.all(got == bits), "%s: %s lands on %s, not %#x" % (out_dt, name, [hex(int(g)) for g in got[:3]], bits)
        assert np.all(r32[e.idx[at]] == np.float32(x0) + np.float32(x1) * np.float32(0.5)), name
    return c


def _finite_inputs(e):
    ok = np.ones(e.n, bool)
    for x in e.xs:
        ok &= np.isfinite(widen(x, e.in_dt))
    if e.init is not None:
        ok &= np.isfinite(e.init)
    return ok


# ------------------------------------------------------------------ device side

def torch_bits_dtype(torch, dt):
    return torch.int32 if dt == F32 else torch.int16


def to_device(torch, fa, e, offsets=None):
    """The inputs of `e` in GuardedBufs: fa_fill_uniform on the device, then the planted values by index_put
    -- the same bytes as e.xs (fill == generator is tests/test_gpu_parity.py's first test).  offsets[k]: the
    16-byte phase of client k in bytes.  Returns (bufs, typed int views)."""
    idx = torch.as_tensor(e.idx, device="cuda")
    bufs, views = [], []
    for k in range(e.D):
        b = GuardedBuf(torch, e.n * ITEM[e.in_dt], offsets[k] if offsets else 0)
        v = b.view(torch_bits_dtype(torch, e.in_dt))
        fa.fill_uniform(b.ptr, e.n, fa_dt(fa, e.in_dt), e.seed, k)
        torch.cuda.synchronize()
        sv = e.vals[k].view(np.int32 if e.in_dt == F32 else np.int16)
        v[idx] = torch.from_numpy(sv).to("cuda")
        bufs.append(b)
        views.append(v)
    return bufs, views


def init_to_device(torch, fa, e, offset=0):
    b = GuardedBuf(torch, e.n * 4, offset)
    v = b.view(torch.int32)
    fa.fill_uniform(b.ptr, e.n, fa.F32, e.seed, 999)
    torch.cuda.synchronize()
    v[torch.as_tensor(e.idx, device="cuda")] = torch.from_numpy(e.init_vals.view(np.int32)).to("cuda")
    return b, v


def device_bits(view, dt):
    """A device int view back on the host as unsigned bits."""
    a = view.cpu().numpy()
    return a.view(BITS[dt])
