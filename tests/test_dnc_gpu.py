"""GPU: the DnC stage (fa.h "DnC stage") on an Aggregator part against tests/dnc_ref.py.

D = 8 owners, n = 4099.  Four lie within 0.05 of a common model, two are honest but noisy (sigma 1), and owners 2 and 5
lie within 0.05 of the model shifted by one common vector of +-1 per element.  A distance rule sees the shifted pair
closer to the crowd (3 n from its honest neighbours) than the noisy owners (4 n): Multi-Krum at f = 2 drops the noisy
two and keeps the pair, which is asserted first on the CPU reference.  The centred buckets have 1.5 n of variance
along the shift against 0.9 n along either noisy owner, so DnC's direction is the shift and the pair projects three
times as far on it as anyone else.
"""
import numpy as np
import pytest

import dnc_ref as R
import krum_ref as K
import server_opt_ref as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
D, N, SHIFTED, NOISY = 8, 4099, (2, 5), (0, 6)
KEPT = [k not in SHIFTED for k in range(D)]


def owners(kind, seed=0xD1C):
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, N).astype(F32)
    v = rng.choice([-1.0, 1.0], N).astype(F32)
    xs = []
    for k in range(D):
        x = g + F32(1.0 if k in NOISY else 0.05) * rng.standard_normal(N).astype(F32)
        xs.append(K.round_out((x + v if k in SHIFTED else x).astype(F32), kind))
    return xs


def reduce_selected(fa, torch, xs, dt, w, sel):
    """fa.reduce_device over the selected owners with fa.krum_weights: the bits the part must give."""
    wp, inc, bits = fa.krum_weights(w, sel), np.flatnonzero(sel), np.int32 if dt == fa.F32 else np.int16
    dev = [torch.from_numpy(np.ascontiguousarray(xs[k]).view(bits)).cuda() for k in inc]
    out = torch.from_numpy(np.zeros(N, bits)).cuda()
    fa.reduce_device(dev, wp[inc], N, dt, out, dt, fa.FEDAVG)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def round_of(agg, xs, w, drop):
    """One round of part 1; its report must be dnc_ref on the reported Gram matrix, bit for bit."""
    for k, x in enumerate(xs):
        agg.submit(1, k, x, w[k])
    out = agg.finalize(1)
    G, s, sel = agg.dnc_round(1)
    rs, rsel = R.dnc_select(G, drop)
    assert np.array_equal(s.view(np.uint64), rs.view(np.uint64)), (s, rs)
    assert sel.tolist() == rsel.tolist(), (sel, rsel)
    return out, s, sel


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_dnc_removes_the_shifted_pair_that_krum_keeps(fa, O, torch_gpu, kind):
    xs, w, dt = owners(kind), O.weights(D), {"f32": fa.F32, "bf16": fa.BF16}[kind]
    _, ksel = K.krum_select(K.distances(xs, kind), 2)
    assert ksel[list(SHIFTED)].any(), ksel  # the premise: Multi-Krum at f = 2 keeps at least one of the pair
    with fa.Aggregator(1) as agg:
        agg.define(1, N, dt, dt, D)
        agg.set_dnc(2, part_id=1)
        out, s, sel = round_of(agg, xs, w, 2)
    assert sel.tolist() == KEPT, (s, sel)
    got = np.ascontiguousarray(out).view(np.int32 if kind == "f32" else np.int16)
    assert np.array_equal(got, reduce_selected(fa, torch_gpu, xs, dt, w, sel))


def test_drop_0_is_plain_fedavg(fa, O, torch_gpu):
    xs, w = owners("f32"), O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        agg.set_dnc(0, part_id=1)
        out, s, sel = round_of(agg, xs, w, 0)
    assert sel.all() and s[list(SHIFTED)].min() > 2 * np.delete(s, SHIFTED).max(), s
    K.assert_bits(out, O.fedavg(xs, w), "drop 0")


def test_dnc_aggregate_feeds_the_server_optimizer(fa, O, torch_gpu):
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    xs, w = owners("f32"), O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, N, fa.F32, fa.F32, D)
        agg.set_server_opt(S.ADAM, part_id=1, **hp)
        agg.set_dnc(2, part_id=1)
        x0 = np.random.default_rng(9).uniform(-1, 1, N).astype(F32)
        agg.set_server_opt_state(1, x=x0)
        out, s, sel = round_of(agg, xs, w, 2)
        assert sel.tolist() == KEPT, (s, sel)
        ref = S.step(S.ADAM, K.aggregate(O, xs, "f32", w, sel), x0, np.zeros(N, F32), np.zeros(N, F32), **hp)
        K.assert_bits(out, ref[0], "the stepped model")
