"""GPU: the Krum distance pass (fa_krum.hip) at every D from 2 to 128, in every lane regime, and at the edges of
its fp32 subtraction.

The pass cuts the D x D pair triangle three ways, by B = ceil(D / 4) and NB = B (B + 1) / 2 (REGIMES below restates
fa_krum.hip's krum_geom and launch_pairdist_nbl): the tile size E, the S = 256 / NB slices of lanes that share a
tile, and, beyond 256 blocks, the 2 or 3 blocks a lane owns.  A mistake in one of them gives a wrong or stale Q_ab
for a few pairs at some D and changes nothing but whom Krum selects, so:

1. the sweep runs every D on lattice inputs (krum_ref.lattice): x_k[i] = scale c_k u_i with small integers u_i,
   so Q_ab = scale^2 (c_a - c_b)^2 sum u_i^2 and every term and partial sum of any order is an exact integer times
   scale^2.  The kernel must return those bits, no tolerance; for f32 the c_k are a Sidon sequence, so all
   entries differ and a sum routed to the wrong slot, block or mirror shows at a known (a, b).  Proved on the host
   in tests/test_krum_cpu.py;
2. real-valued rounds (test_krum_gpu's clients and its four assertions, the bound n * 2^-53 * exact of fa.h) run
   one D per regime that had none;
3. rule 1's "d = fl32(x_a - x_b), then an exact fp64 square" is checked where a plausible wrong kernel differs:
   subnormal inputs and differences (a flushed one gives 0), a difference that overflows fp32 (+inf, not 3.6e77),
   inf - inf = NaN, inf - -inf = +inf, and a NaN confined to its client's row -- each planted in the head, the
   first tile, the last partial tile and the tail, so that every staging path carries it.

No expected value comes from the code under test: the closed form and K.pair_sumsq are the references.
"""
import math

import numpy as np
import pytest

import krum_ref as K
from guarded import GuardedBuf, assert_unchanged, snapshot
from test_krum_gpu import SEED, bits64, check_q, check_round, fa_dt, honest_flags, make_clients, submit_all

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = ["f32", "bf16", "f16"]
N = K.LATTICE_N
VEC = {"f32": 4, "bf16": 8, "f16": 8}
LAYOUTS = ["phase 1", "phase 0", "mixed"]

# (D from, D to, tile E, blocks per lane): fa_krum.hip's geometry, restated
REGIMES = [(2, 4, 2048, 1), (5, 8, 1024, 1), (9, 16, 512, 1), (17, 32, 256, 1), (33, 60, 128, 1), (61, 64, 128, 1),
           (65, 88, 64, 1), (89, 124, 64, 2), (125, 128, 64, 3)]
TILES = sorted({r[2] for r in REGIMES})


def geometry(D):
    """(B, NB, E, S, NBL) of D clients: the restatement the size conditions below are asserted from."""
    B = (D + 3) // 4
    NB = B * (B + 1) // 2
    E, NBL = next((e, q) for lo, hi, e, q in REGIMES if lo <= D <= hi)
    return B, NB, E, (min(256 // NB, E // 4) if NB <= 256 else 1), NBL


def test_the_restated_geometry_and_the_sweep_size():
    """The table the module was written from, and what the sweep's n must give at a shared phase of 1 element."""
    slices = [geometry(D)[3] for D in range(2, 129)]
    assert sorted(set(slices), reverse=True) == [256, 85, 42, 25, 17, 12, 9, 7, 5, 4, 3, 2, 1]
    for D in range(2, 129):
        B, NB, E, S, NBL = geometry(D)
        assert 4 * B * (E + 4) <= 8704 and (E == 2048 or 4 * B * (2 * E + 4) > 8704)  # the largest tile that fits
        assert NBL == (NB + 255) // 256 and (S == 1 or NBL == 1) and S * NB <= NBL * 256
    assert [D for D in range(2, 129) if geometry(D)[4] == 2] == list(range(89, 125))
    for V in (4, 8):
        head = V - 1  # from phase 1 to the 16-byte boundary
        nvec, tail = divmod(N - head, V)
        assert head > 0 and tail > 0 and nvec > 0
        for E in TILES:
            assert nvec % (E // V) != 0, (V, E)  # the last tile is partial
        assert -(-nvec // (2048 // V)) >= 2 and -(-nvec // (64 // V)) >= 60
    assert N % 64 % 4 != 0  # the element form's last tile ends inside a group of 4


# ------------------------------------------------------------------ the lattice on the device

def phases(kind, layout):
    V = VEC[kind]
    return [1 if layout == "phase 1" else 0 if layout == "phase 0" else k % V for k in range(K.LATTICE_CLIENTS)]


class Device:
    """The 128 lattice clients of (kind, scale) in GuardedBufs at the phases of `layout`."""

    def __init__(self, torch, kind, layout, scale):
        self.kind, self.layout = kind, layout
        self.c, self.u, self.xs = K.lattice(N, kind, scale)
        self.Q = K.lattice_distances(self.c, self.u, scale)
        item = 4 if kind == "f32" else 2
        self.bufs, self.views, self.snaps = [], [], []
        for x, o in zip(self.xs, phases(kind, layout)):
            b = GuardedBuf(torch, N * item, o * item)
            v = b.view(torch.int32 if kind == "f32" else torch.int16)
            v.copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if kind == "f32" else np.int16)))
            self.bufs.append(b)
            self.views.append(v)
            self.snaps.append(snapshot(v))
        torch.cuda.synchronize()
        self.ptrs = [b.ptr for b in self.bufs]

    def check_untouched(self, D=K.LATTICE_CLIENTS):
        for k in range(D):
            what = "%s %s client %d" % (self.kind, self.layout, k)
            self.bufs[k].check(what)
            assert_unchanged(self.views[k], self.snaps[k], what)


@pytest.fixture(scope="module")
def device(torch_gpu):
    made = {}

    def get(kind, layout, scale=1.0):
        key = (kind, layout, scale)
        if key not in made:
            made[key] = Device(torch_gpu, kind, layout, scale)
        return made[key]

    yield get
    made.clear()


def assert_matrix_bits(Q, exp, what):
    """Q is the matrix `exp` bit for bit (NaN where it has NaN), hence bit-symmetric with a +0 diagonal."""
    D = exp.shape[0]
    assert Q.shape == (D, D), (what, Q.shape)
    assert not bits64(np.diag(Q)).any(), what + ": the diagonal is not +0"
    assert np.array_equal(bits64(Q), bits64(Q.T)), what + ": not bit-symmetric"
    bad = (bits64(Q) != bits64(exp)) & ~(np.isnan(Q) & np.isnan(exp))
    if bad.any():
        at = np.argwhere(np.triu(bad))
        raise AssertionError("%s: %d of %d pairs differ, first %s" % (what, len(at), D * (D - 1) // 2, [
            "Q[%d, %d] = %r, expected %r" % (a, b, Q[a, b], exp[a, b]) for a, b in at[:4]]))


def sweep(fa, dev, Ds, n, ctx, Q=None):
    Q = dev.Q if Q is None else Q
    for D in Ds:
        got = fa.pairdist_device(dev.ptrs[:D], n, fa_dt(fa, dev.kind), ctx=ctx)
        assert_matrix_bits(got, Q[:D, :D], "%s %s n %d D %d %s" % (dev.kind, dev.layout, n, D, geometry(D)))


# ------------------------------------------------------------------ 2. every D, per kind

MIXED_DS = sorted(set(range(2, 17)) | set(range(17, 57, 4)) | set(range(57, 129)))


@pytest.mark.parametrize("kind", KINDS)
def test_every_D_is_bit_exact_on_the_lattice(fa, torch_gpu, device, kind):
    """D ascending within a layout: the partials scratch a call leaves behind then belongs to another D, whose
    slots name other pairs, so a pair the kernel fails to write cannot come out right by staleness."""
    with fa.Aggregator(1) as agg:
        for layout in LAYOUTS:
            dev = device(kind, layout)
            sweep(fa, dev, MIXED_DS if layout == "mixed" else range(2, 129), N, agg)
    dev = device(kind, "phase 1")
    sweep(fa, dev, (2, 61, 89, 127), N, None)  # without a context: scratch of the call's own
    for layout in LAYOUTS:
        device(kind, layout).check_untouched()


@pytest.mark.parametrize("kind", KINDS)
def test_every_D_at_small_n(fa, torch_gpu, device, kind):
    """Fewer elements than one group, a bucket shorter than the head, one vector, a single partial tile."""
    dev = device(kind, "phase 1")
    with fa.Aggregator(1) as agg:
        for n in (1, 3, VEC[kind], 67):
            sweep(fa, dev, range(2, 129), n, agg, K.lattice_distances(dev.c, dev.u[:n]))
    dev.check_untouched()


@pytest.mark.parametrize("kind", KINDS)
def test_capped_grid_strides_the_tiles(fa, torch_gpu, device, kind):
    """3 workgroups: each accumulates several tiles (the last of them partial for one) before its flush."""
    with fa.Aggregator(1) as agg:
        agg.set_tuning(max_blocks=3)
        for layout in LAYOUTS:
            sweep(fa, device(kind, layout), (12, 24, 70, 100, 127), N, agg)
    for layout in LAYOUTS:
        device(kind, layout).check_untouched()


# ------------------------------------------------------------------ 3. real-valued rounds, one D per regime

@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("D,f", [(12, 3), (20, 6), (50, 20), (61, 20), (88, 40), (89, 40), (124, 60), (125, 60)])
def test_multi_krum_round_in_every_regime(fa, O, torch_gpu, D, f, kind):
    n = 4099 if D <= 50 else 1031
    assert -(-n // 64) >= 16
    xs = make_clients(n, D, f, kind, SEED + 11 * n + D)
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa_dt(fa, kind), fa_dt(fa, kind), D)
        agg.set_krum(f, None, 1)
        submit_all(agg, 1, xs, w)
        out = agg.finalize(1)
        what = "%s D %d f %d n %d" % (kind, D, f, n)
        _, scores, _, _ = check_round(agg, O, 1, out, xs, kind, kind, w, f, D - f, what, expect=honest_flags(D, f))
        honest = honest_flags(D, f)
        assert scores[~honest].min() > 600 * scores[honest].max(), (what, scores)


# ------------------------------------------------------------------ 4. the fp32 subtraction's edges

EDGE_DS = (5, 70, 100, 128)  # sliced, and 1, 2 and 3 blocks per lane


@pytest.mark.parametrize("kind", KINDS)
def test_subnormal_inputs_and_differences_are_kept(fa, torch_gpu, device, kind):
    scale = K.SUBNORMAL_SCALE[kind]
    tiny = K.SMALLEST_NORMAL[kind]
    with fa.Aggregator(1) as agg:
        for layout in ("phase 1", "mixed"):
            dev = device(kind, layout, scale)
            for k, x in enumerate(dev.xs):  # the inputs really are subnormal in their type
                w = np.abs(K.widen(x, kind).astype(np.float64))
                if kind != "bf16" or k < 64:
                    assert (w < tiny).all() and ((w > 0).all() or dev.c[k] == 0), (kind, k)
                else:  # bf16 has 128 subnormal steps and |c u| reaches 254: the rest fill the first normal binade
                    assert (w < 2 * tiny).all() and (w[np.abs(dev.u) == 1] < tiny).all(), (kind, k)
            assert dev.Q[0, 1] == scale * scale * float((dev.u * dev.u).sum()) > 0
            sweep(fa, dev, EDGE_DS, N, agg)
            dev.check_untouched()


def f32_bits(v):
    return int(np.asarray([v], F32).view(np.int32)[0])


def planted(fa, dev, ctx, D, plants):
    """The matrix of the first D clients with plants = [(client, index, value)] in place of the lattice's values,
    and the expected one: the closed form, the rows of the planted clients by K.pair_sumsq (exactly rounded; where
    it is finite every other term is an integer below 2^53, far under half an ulp of the planted square, so any
    summation order gives these bits)."""
    xs = [x.copy() for x in dev.xs[:D]]
    try:
        for k, j, v in plants:
            xs[k][j] = v
            dev.views[k][j] = f32_bits(v)
        got = fa.pairdist_device(dev.ptrs[:D], N, fa.F32, ctx=ctx)
    finally:
        for k, j, _ in plants:
            dev.views[k][j] = f32_bits(dev.xs[k][j])
    exp = dev.Q[:D, :D].copy()
    for k in sorted({k for k, _, _ in plants}):
        for b in range(D):
            if b != k:
                exp[k, b] = exp[b, k] = K.pair_sumsq(xs[k], xs[b])
    return got, exp


def places():
    """Element indices in the head, the first tile, the last partial tile (of every tile size) and the tail of the
    f32 bucket at phase 1, and one more for a second plant."""
    head = 3
    nvec, tail = divmod(N - head, 4)
    tail0 = head + 4 * nvec
    last_tile = head + (nvec - nvec % 512) * 4  # the first element of the last tile at E = 2048, hence at every E
    assert tail0 - last_tile < 64 and tail > 0
    return {"head": 1, "first tile": head + 37, "last partial tile": tail0 - 3, "tail": N - 1}, head + 300


SPECIALS = ["overflow", "inf - inf", "inf - -inf", "nan"]


@pytest.mark.parametrize("special", SPECIALS)
def test_special_values_follow_the_fp32_subtraction(fa, torch_gpu, device, special):
    dev = device("f32", "phase 1")
    inf = np.inf
    with fa.Aggregator(1) as agg:
        for D in EDGE_DS:
            for place, j in places()[0].items():
                what = "%s in the %s, D %d" % (special, place, D)
                if special == "overflow":
                    got, exp = planted(fa, dev, agg, D, [(1, j, F32(3e38)), (2, j, F32(-3e38))])
                    assert got[1, 2] == inf, (what, got[1, 2])  # fl32(3e38 - -3e38) = +inf, not 3.6e77 in fp64
                    rest = np.delete(got[1:3], [1, 2], axis=1)
                    assert np.isfinite(rest).all() and (rest > 8.9e76).all(), what
                    others = int((dev.u * dev.u).sum()) - int(dev.u[j]) ** 2  # the closed form without element j
                    for k, v in ((1, F32(3e38)), (2, F32(-3e38))):
                        for b in (0, 3, D - 1):
                            d = float(F32(v - dev.xs[b][j]))
                            want = math.fsum([float(int(dev.c[k] - dev.c[b]) ** 2 * others), d * d])
                            assert bits64(got[k, b]) == bits64(want), (what, k, b, got[k, b], want)
                elif special == "inf - inf":
                    got, exp = planted(fa, dev, agg, D, [(3, j, F32(inf)), (4, j, F32(inf))])
                    assert np.isnan(got[3, 4]) and (np.delete(got[3:5], [3, 4], axis=1) == inf).all(), what
                elif special == "inf - -inf":
                    got, exp = planted(fa, dev, agg, D, [(3, j, F32(inf)), (0, j, F32(-inf))])
                    assert got[3, 0] == inf and (np.delete(got[3], 3) == inf).all(), what
                else:
                    got, exp = planted(fa, dev, agg, D, [(D - 1, j, F32(np.nan))])
                    assert np.isnan(np.delete(got[D - 1], D - 1)).all() and bits64(got[D - 1, D - 1]) == 0, what
                    assert np.isfinite(got[:D - 1, :D - 1]).all(), what
                assert_matrix_bits(got, exp, what)  # every entry without a special client is the closed form's
    dev.check_untouched()


def test_inf_pairs_at_two_indices(fa, torch_gpu, device):
    """Clients 3 and 4 hold +inf at one index, clients 3 and 0 +inf and -inf at another: NaN for (3, 4) only."""
    dev = device("f32", "phase 1")
    where, other = places()
    inf = np.inf
    with fa.Aggregator(1) as agg:
        for D in EDGE_DS:
            for place, j in where.items():
                what = "two infs, the %s, D %d" % (place, D)
                got, exp = planted(fa, dev, agg, D, [(3, j, F32(inf)), (4, j, F32(inf)), (3, other, F32(inf)),
                                                      (0, other, F32(-inf))])
                assert np.isnan(got[3, 4]) and got[3, 0] == inf and got[4, 0] == inf, what
                assert (np.delete(got[[0, 3, 4]], [0, 3, 4], axis=1) == inf).all(), what
                assert_matrix_bits(got, exp, what)
    dev.check_untouched()
