"""GPU: the sorting kernels (fa_trimmed.hip, fa_centered.hip, fa_sortnet.h) at every D, window, form and key
pattern, every bit.

* the trimmed mean at every D = 1..128: every dtype pair, the trims of sort_cols.trim_set, three pointer layouts
  (all at 16-byte phase 0: the vector form; a shared phase of one element: head + vectors + tail; mixed phases:
  the element form), n = 67 and 4099, normals with bulyan_ref.special_columns planted at the start, the middle
  and the end, against trimmed_ref;
* the two-valued column families of tests/sort_cols.py (every 0-1 pattern of D <= 16, at most two lows or highs
  and the threshold columns of random permutations up to D = 64, every split of the lows between the halves of
  the wide form) through fa_trimmed_device against the closed form, which needs no sort, and through
  fa_centered_device (keep = D: the same closed form; keep < D: bulyan_ref), in fp32, bf16 and fp16; above
  D = 16 once more at every trim, which puts a window edge at every sorted position;
* the centred mean at every keep of nine theta on the slide columns (the window start is known: every reachable
  one occurs, tests/test_bulyan_cpu.py), permutations, normals and the special columns;
* the structured columns through the grid-stride loops of a grid capped at three workgroups.

Every buffer is a GuardedBuf.  After each launch the output's guards are checked on the host and every client's
guards and payload against the bytes they held after the upload, on the device; after the launches of one upload
the clients' guards are checked against the pattern itself and their payloads against the snapshots.  Where the
expected value is NaN a NaN is required, everything else is bit for bit.
"""
import numpy as np
import pytest

import bulyan_ref as B
import sort_cols as S
import test_centered_gpu as C
import trimmed_ref as T
from guarded import PAIRS, GuardedBuf, assert_unchanged

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = ["f32", "bf16", "f16"]
NS = [67, 4099]  # a head alone; a head, vectors and a tail
# eight D per test up to 64, four above: a few seconds each
D_RANGES = [(lo, lo + 7) for lo in range(1, 65, 8)] + [(lo, lo + 3) for lo in range(65, 129, 4)]
STRUCTURED_DS = S.DS_EXHAUSTIVE + S.DS_NETWORK + S.DS_WIDE


def outs_of(in_kind):
    return [o for i, o in PAIRS if i == in_kind]


def out_phase(offsets, in_kind, okind):
    """The output shares the clients' phase in bytes where they share one, else it sits at phase 0."""
    ophase = offsets[0] * C.ITEM[in_kind] if len(set(offsets)) == 1 else 0
    return 0 if ophase % C.ITEM[okind] else ophase


class Clients:
    """One upload of the client buckets (rows of `kind`) into guarded buffers at the given 16-byte phases."""

    def __init__(self, torch, xs, kind, offsets):
        self.torch, self.kind, self.n = torch, kind, xs[0].size
        self.bufs, self.views, self.snaps = C.upload(torch, xs, kind, offsets)
        self.ptrs = [b.ptr for b in self.bufs]
        self.whole = [b.base.clone() for b in self.bufs]  # guards and payload as uploaded

    def after_launch(self, what):
        """Guards and payload of every client, on the device; a difference is named by close()."""
        torch = self.torch
        bad = torch.zeros((), dtype=torch.bool, device="cuda")
        for b, w in zip(self.bufs, self.whole):
            bad |= (b.base != w).any()
        if bool(bad):
            self.close(what)
            raise AssertionError("%s: a client allocation changed outside its guards and payload" % what)

    def close(self, what):
        """The guards against the pattern itself and the payload against its snapshot, client by client."""
        for k, b in enumerate(self.bufs):
            b.check("%s, client %d" % (what, k))
            assert_unchanged(self.views[k], self.snaps[k], "%s, client %d" % (what, k))


def launch(fa, torch, cl, in_kind, okind, ophase, ref_f32, what, trim=None, keep=None, ctx=None):
    """One launch into a fresh guarded output: the bits, the output's guards, the clients."""
    out = GuardedBuf(torch, cl.n * C.ITEM[okind], ophase)
    if keep is None:
        fa.trimmed_device(cl.ptrs, cl.n, C.fa_dt(fa, in_kind), out.ptr, C.fa_dt(fa, okind), trim=trim, ctx=ctx)
    else:
        fa.centered_device(cl.ptrs, cl.n, C.fa_dt(fa, in_kind), out.ptr, C.fa_dt(fa, okind), keep=keep, ctx=ctx)
    torch.cuda.synchronize()
    B.assert_bits(C.read_out(torch, out, okind, cl.n), B.round_out(ref_f32, okind), what)
    out.check(what)
    cl.after_launch(what)


def rows_of(x, kind):
    """The clients' buckets of `kind` from the fp32 matrix x (D, n)."""
    return [B.round_out(np.ascontiguousarray(r), kind) for r in x]


# ------------------------------------------------------------------ every D for the trimmed mean

@pytest.mark.parametrize("in_kind", KINDS)
@pytest.mark.parametrize("d_lo,d_hi", D_RANGES)
def test_trimmed_mean_at_every_D(fa, torch_gpu, d_lo, d_hi, in_kind):
    torch = torch_gpu
    for D in range(d_lo, d_hi + 1):
        for n in NS:
            xs = C.make_inputs(D, n, in_kind)
            wide = [B.widen(x, in_kind) for x in xs]
            refs = {t: T.trimmed_f32(wide, t) for t in {T.resolve(trim, D) for trim in S.trim_set(D)}}
            for name, offsets in C.layouts(D, in_kind).items():
                cl = Clients(torch, xs, in_kind, offsets)
                for okind in outs_of(in_kind):
                    for trim in S.trim_set(D):
                        what = "D %d trim %d n %d %s -> %s, %s" % (D, trim, n, in_kind, okind, name)
                        launch(fa, torch, cl, in_kind, okind, out_phase(offsets, in_kind, okind),
                               refs[T.resolve(trim, D)], what, trim=trim)
                cl.close("D %d n %d %s %s" % (D, n, in_kind, name))


# ------------------------------------------------------------------ the two-valued families and the permutations

_CENTRED = {}  # (D, pair, keep) -> the fp32 reference; the values are exact in every kind, so the kinds share it


def structured(D, pair):
    """(x (D, n) fp32, z (C,)): the two-valued columns of `pair`, then 64 permutations as values; n % 8 == 3."""
    mask, z = S.zero_one(D)
    return np.concatenate([S.values(mask, pair), S.perm_values(D)], axis=1), z


@pytest.mark.parametrize("in_kind", KINDS)
@pytest.mark.parametrize("D", STRUCTURED_DS)
def test_two_valued_columns_have_the_closed_form(fa, torch_gpu, D, in_kind):
    """fa_trimmed_device against the closed form (the permutations: against trimmed_ref, their sums are exact)."""
    torch = torch_gpu
    for pair in S.PAIRS01:
        x, z = structured(D, pair)
        perms = list(x[:, z.size:])
        refs = {}
        for trim in S.trims_for(D):
            t = T.resolve(trim, D)
            if t not in refs:
                refs[t] = np.concatenate([S.closed_form(D, t, z, pair), T.trimmed_f32(perms, t)])
        xs = rows_of(x, in_kind)
        for name, offsets in C.layouts(D, in_kind).items():
            cl = Clients(torch, xs, in_kind, offsets)
            for okind in outs_of(in_kind):
                for trim in S.trims_for(D):
                    what = "D %d %s trim %d %s -> %s, %s" % (D, pair, trim, in_kind, okind, name)
                    launch(fa, torch, cl, in_kind, okind, out_phase(offsets, in_kind, okind), refs[T.resolve(trim, D)],
                           what, trim=trim)
            cl.close("D %d %s %s %s" % (D, pair, in_kind, name))


@pytest.mark.parametrize("in_kind", KINDS)
@pytest.mark.parametrize("D", S.DS_NETWORK + S.DS_WIDE)
def test_two_valued_columns_at_every_trim(fa, torch_gpu, D, in_kind):
    """The sums of these columns are exact, so a pair of sorted positions left in the wrong order shows only where
    a window edge falls between the two: trim t puts the edges at t and D - t, and every trim puts one at every
    position.  fp32 out; fp32 in at phase 0 and at mixed phases, the 16-bit inputs at phase 0."""
    torch = torch_gpu
    trims = list(range((D - 1) // 2 + 1))
    for pair in S.PAIRS01:
        x, z = structured(D, pair)
        perms = list(x[:, z.size:])
        xs = rows_of(x, in_kind)
        for name, offsets in C.layouts(D, in_kind).items():
            if name == "shared phase 1" or (name == "mixed" and in_kind != "f32"):
                continue
            cl = Clients(torch, xs, in_kind, offsets)
            for t in trims:
                ref = np.concatenate([S.closed_form(D, t, z, pair), T.trimmed_f32(perms, t)])
                launch(fa, torch, cl, in_kind, "f32", 0, ref, "D %d %s trim %d %s, %s" % (D, pair, t, in_kind, name), trim=t)
            cl.close("D %d %s %s %s" % (D, pair, in_kind, name))


@pytest.mark.parametrize("in_kind", KINDS)
@pytest.mark.parametrize("D", STRUCTURED_DS)
def test_two_valued_columns_through_the_centred_mean(fa, torch_gpu, D, in_kind):
    """keep = D cannot move the window: the trim-0 closed form.  keep < D: bulyan_ref."""
    torch = torch_gpu
    for pair in S.PAIRS01:
        x, z = structured(D, pair)
        for keep in S.keeps_for(D):
            if (D, pair, keep) not in _CENTRED:
                if keep == D:
                    ref = np.concatenate([S.closed_form(D, 0, z, pair), T.trimmed_f32(list(x[:, z.size:]), 0)])
                else:
                    ref = B.centered_f32(list(x), keep)[0]
                _CENTRED[D, pair, keep] = ref
        xs = rows_of(x, in_kind)
        for name, offsets in C.layouts(D, in_kind).items():
            if name == "shared phase 1":
                continue  # the vector form at phase 0, the element form at mixed phases
            cl = Clients(torch, xs, in_kind, offsets)
            for okind in outs_of(in_kind):
                for keep in S.keeps_for(D):
                    what = "D %d %s keep %d %s -> %s, %s" % (D, pair, keep, in_kind, okind, name)
                    launch(fa, torch, cl, in_kind, okind, 0, _CENTRED[D, pair, keep], what, keep=keep)
            cl.close("D %d %s %s %s" % (D, pair, in_kind, name))


# ------------------------------------------------------------------ every keep for the centred mean

_EVERY_KEEP = {}  # (theta, kind) -> (the clients' buckets, {keep: the fp32 reference})


def every_keep_case(theta, kind):
    if (theta, kind) not in _EVERY_KEEP:
        slide, _ = S.slide_columns(theta)
        rng = np.random.default_rng(S.SEED + 17 * theta)
        cols = B.special_columns(theta)
        normals = rng.normal(size=(theta, 203 + (-slide.shape[1]) % 8)).astype(F32)
        for base in (0, normals.shape[1] - len(cols)):
            for c, col in enumerate(cols):
                normals[:, base + c] = col
        x = np.concatenate([slide, S.perm_values(theta), normals], axis=1)
        assert x.shape[1] % 8 == 3
        xs = rows_of(x, kind)
        wide = [B.widen(r, kind) for r in xs]
        _EVERY_KEEP[theta, kind] = xs, {keep: B.centered_f32(wide, keep)[0] for keep in range(1, theta + 1)}
    return _EVERY_KEEP[theta, kind]


@pytest.mark.parametrize("in_kind,layout", [("f32", "phase 0"), ("f32", "shared phase 1"), ("f32", "mixed"),
                                            ("bf16", "phase 0"), ("f16", "phase 0")])
@pytest.mark.parametrize("theta", S.SLIDE_THETAS)
def test_centred_mean_at_every_keep(fa, torch_gpu, theta, in_kind, layout):
    torch = torch_gpu
    xs, refs = every_keep_case(theta, in_kind)
    offsets = C.layouts(theta, in_kind)[layout]
    cl = Clients(torch, xs, in_kind, offsets)
    for okind in outs_of(in_kind):
        for keep in range(1, theta + 1):
            what = "theta %d keep %d %s -> %s, %s" % (theta, keep, in_kind, okind, layout)
            launch(fa, torch, cl, in_kind, okind, out_phase(offsets, in_kind, okind), refs[keep], what, keep=keep)
    cl.close("theta %d %s %s" % (theta, in_kind, layout))


# ------------------------------------------------------------------ a capped grid

@pytest.mark.parametrize("D,trim,keep", [(16, 3, 9), (128, 31, 64)])
def test_structured_columns_through_a_capped_grid(fa, torch_gpu, D, trim, keep):
    """Three workgroups: every 0-1 pattern of D = 16 and every split of D = 128 through the grid-stride loops."""
    torch = torch_gpu
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=3)
        for pair in S.PAIRS01:
            x, z = structured(D, pair)
            cl = Clients(torch, rows_of(x, "f32"), "f32", [0] * D)
            ref = np.concatenate([S.closed_form(D, trim, z, pair), T.trimmed_f32(list(x[:, z.size:]), trim)])
            launch(fa, torch, cl, "f32", "f32", 0, ref, "3 workgroups, D %d %s trim %d" % (D, pair, trim), trim=trim, ctx=agg)
            launch(fa, torch, cl, "f32", "f32", 0, B.centered_f32(list(x), keep)[0],
                   "3 workgroups, D %d %s keep %d" % (D, pair, keep), keep=keep, ctx=agg)
            cl.close("3 workgroups, D %d %s" % (D, pair))
