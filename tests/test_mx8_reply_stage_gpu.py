"""GPU: the MX8 reply stage through a context (fa_set_mx8_reply, fa_finalize_mx8, fa_copy_mx8, fa_mx8_reply_stats).

What the part's output must be without the stage (y) comes from the oracle for FedAvg and, for the other modes and
stages, from a second aggregator without the reply stage that is fed the same receipts; tests/mx8_reply_ref.py chains
rules 1-5 over the rounds from it.  Every round's codes and output are compared bit for bit.  D = 3, n = 4099.
"""
import numpy as np
import pytest

import clip_ref as R
import mx8_ref as M
import mx8_reply_ref as P
import server_opt_ref as S

pytestmark = pytest.mark.gpu

F32, I8, U8 = np.float32, np.int8, np.uint8
N, D = 4099, 3


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def make_clients(n, kind, seed, around=None, step=0.02):
    """D clients near `around` (fp32 values; None: a fresh uniform model), so a round moves the model a little."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, n).astype(F32) if around is None else around
    return [R.round_out((base + F32(step) * rng.standard_normal(n).astype(F32)).astype(F32), kind) for _ in range(D)]


def plain_aggregate(O, xs, kind, w):
    if kind == "bf16":
        return O.fedavg([np.ascontiguousarray(x) for x in xs], w, out_dtype="f32")
    return O.fedavg([R.widen(x, kind) for x in xs], w)


def submit_all(agg, part, xs, w):
    for k in range(D):
        agg.submit(part, k, xs[k], w[k])


def state_error(fa, fn, *a):
    with pytest.raises(fa.FaError) as ei:
        fn(*a)
    assert ei.value.code == fa.ERR_STATE, str(ei.value)
    return str(ei.value)


def check_round(agg, part, want, kind, what, finalize="mx8"):
    """Ends the round and compares codes and output with `want` = (q, e, g') of the restatement."""
    q, e = agg.finalize_mx8(part) if finalize == "mx8" else (None, None)
    out = agg.finalize(part) if finalize == "full" else agg.copy_output(part)
    if q is None:
        q, e = agg.copy_mx8(part)
    assert np.array_equal(e, want[1]), (what, np.flatnonzero(e != want[1])[:8])
    assert np.array_equal(q, want[0]), (what, np.flatnonzero(q != want[0])[:8])
    R.assert_bits(out, want[2], what)
    return q, e, out


# ------------------------------------------------------------------ bootstrap, FedAvg over rounds

def test_bootstrap_round(fa, O, torch_gpu):
    part, w = 1, O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(part, N, fa.F32, fa.F32, D)
        agg.set_mx8_reply(True, part)
        assert agg.mx8_reply_stats(part) == 0
        state_error(fa, agg.copy_mx8, part)
        xs = make_clients(N, "f32", 1)
        submit_all(agg, part, xs, w)
        assert agg.host_read_kept(part) == 0
        assert "bootstrap" in state_error(fa, agg.finalize_mx8, part)
        assert agg.progress(part) == (D, 0)  # refused before any work: the round is intact
        y = plain_aggregate(O, xs, "f32", w)
        R.assert_bits(agg.finalize(part), y, "the bootstrap's output is y")
        state_error(fa, agg.copy_mx8, part)  # the round had no codes
        assert agg.mx8_reply_stats(part) == 0
        # reduced by hand, the bootstrap still refuses the codes and leaves the round to fa_finalize
        agg.set_mx8_reply(False, part)
        agg.set_mx8_reply(True, part)  # off and on: `sent` is gone
        submit_all(agg, part, xs, w)
        agg.reduce(part)
        assert agg.progress(part) == (D, D)
        state_error(fa, agg.finalize_mx8, part)
        R.assert_bits(agg.finalize(part), y, "bootstrap again after off and on")
        # without the stage: both entries refuse
        agg.set_mx8_reply(False, part)
        submit_all(agg, part, xs, w)
        assert "fa_set_mx8_reply" in state_error(fa, agg.finalize_mx8, part)
        state_error(fa, agg.mx8_reply_stats, part)
        R.assert_bits(agg.finalize(part), y, "stage off")


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_three_rounds_of_fedavg(fa, O, torch_gpu, kind):
    """Rounds 2 and 3 reply in MX8.  An owner who loaded round 1's full reply and adds every decoded reply since (decode
    rule 3, fa_mx8_decode) holds exactly the part's output."""
    part, w = 2, O.weights(D)
    owners = P.Owners(kind)
    with fa.Aggregator(1) as agg:
        agg.set_mx8_reply()  # the context default
        agg.define(part, N, fa_dt(fa, kind), fa_dt(fa, kind), D)
        model = None
        for rnd in range(3):
            xs = make_clients(N, kind, 10 + rnd, model)
            submit_all(agg, part, xs, w)
            y = R.round_out(plain_aggregate(O, xs, kind, w), kind)
            want = owners.round(y)
            if rnd == 0:
                owner = agg.finalize(part)
                R.assert_bits(owner, y, "round 1")
            else:
                q, e, out = check_round(agg, part, want, kind, "%s round %d" % (kind, rnd + 1),
                                        "mx8" if rnd == 1 else "full")
                assert np.abs(q).max() > 64 and len(set(e.tolist())) > 1  # real codes
                assert not np.array_equal(np.ascontiguousarray(out).view(U8), np.ascontiguousarray(y).view(U8)), "lossy"
                with np.errstate(all="ignore"):
                    owner = M.round_out((M.widen(owner, kind) + fa.mx8_decode(q, e)).astype(F32), kind)
                R.assert_bits(owner, out, "the owner's model, round %d" % (rnd + 1))
                assert agg.mx8_reply_stats(part) == 0
            model = R.widen(agg.copy_output(part), kind)


# ------------------------------------------------------------------ beside the other stages

def test_server_optimizer_keeps_the_exact_master(fa, O, torch_gpu):
    """With FedAdam the master, the moments and the step count equal the run without the reply stage bit for bit;
    the output is g' of the stepped model."""
    part, w = 3, O.weights(D)
    hp = dict(lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3)
    owners = P.Owners("f32")
    with fa.Aggregator(1) as agg, fa.Aggregator(1) as twin:
        for a in (agg, twin):
            a.set_server_opt(S.ADAM, **hp)
        agg.set_mx8_reply()
        for a in (agg, twin):
            a.define(part, N, fa.F32, fa.F32, D)
        for rnd in range(3):
            xs = make_clients(N, "f32", 20 + rnd)
            submit_all(agg, part, xs, w)
            submit_all(twin, part, xs, w)
            y = twin.finalize(part)
            want = owners.round(y)
            if rnd == 0:
                R.assert_bits(agg.finalize(part), y, "round 1")
            else:
                check_round(agg, part, want, "f32", "adam round %d" % (rnd + 1))
            sa, st = agg.server_opt_state(part), twin.server_opt_state(part)
            for name, a, b in zip(("x", "m", "v"), sa[:3], st[:3]):
                R.assert_bits(a, b, "%s after round %d" % (name, rnd + 1))
            assert sa[3] == st[3]


def test_clip_reference_is_the_new_model(fa, O, torch_gpu):
    """Clip rule 6 takes widen(g'): after an MX8 round the reference is what the owners hold, and the next round clips
    against it."""
    part, w, C = 4, O.weights(D), 0.5  # updates of norm ~0.02 sqrt(N) = 1.3: clipped
    owners = P.Owners("bf16")
    with fa.Aggregator(1) as agg, fa.Aggregator(1) as twin:
        for a in (agg, twin):
            a.define(part, N, fa.BF16, fa.BF16, D)
            a.set_clip(C, part)
        agg.set_mx8_reply(True, part)
        model = None
        for rnd in range(3):
            xs = make_clients(N, "bf16", 30 + rnd, model)
            submit_all(agg, part, xs, w)
            submit_all(twin, part, xs, w)
            y = twin.finalize(part)
            want = owners.round(y)
            if rnd == 0:
                R.assert_bits(agg.finalize(part), y, "round 1")
            else:
                check_round(agg, part, want, "bf16", "clip round %d" % (rnd + 1))
                assert agg.clip_round(part)[3] > 0
                assert np.array_equal(agg.clip_round(part)[0], twin.clip_round(part)[0])
            R.assert_bits(agg.clip_reference(part), M.widen(owners.sent, "bf16"), "clip reference, round %d" % (rnd + 1))
            twin.set_clip_reference(part, M.widen(owners.sent, "bf16"))  # the twin's owners were sent g' too
            model = M.widen(owners.sent, "bf16")


def test_mx8_receipts_expand_against_the_new_model(fa, O, torch_gpu):
    """Receipts in MX8 and replies in MX8: round 3's relative submits are expanded against round 2's g'."""
    part, w = 5, O.weights(D)
    owners = P.Owners("f32")
    with fa.Aggregator(1) as agg:
        agg.set_mx8()
        agg.set_mx8_reply()
        agg.define(part, N, fa.F32, fa.F32, D)
        for rnd in range(2):
            xs = make_clients(N, "f32", 40 + rnd)
            submit_all(agg, part, xs, w)
            want = owners.round(plain_aggregate(O, xs, "f32", w))
            if rnd == 0:
                agg.finalize(part)
            else:
                check_round(agg, part, want, "f32", "round 2")
        g = owners.sent
        xs = []
        for k in range(D):
            x = (g + F32(0.05) * np.random.default_rng(50 + k).standard_normal(N).astype(F32)).astype(F32)
            q, e = M.encode((x - g).astype(F32))
            agg.submit_mx8(part, k, q, e, w[k])
            xs.append(M.expand(q, e, 0, "f32", g, "f32"))
        check_round(agg, part, owners.round(plain_aggregate(O, xs, "f32", w)), "f32", "round 3")


def configure_trimmed(fa, a, part):
    a.define(part, N, fa.F32, fa.F32, D, mode=fa.TRIMMED, trim=1)


def configure_krum(fa, a, part):
    a.define(part, N, fa.F32, fa.F32, D)
    a.set_krum(0, 2, part)


def configure_noise(fa, a, part):
    a.define(part, N, fa.F32, fa.F16, D)
    a.set_noise(0.01, 0x5EED, part)


@pytest.mark.parametrize("configure,okind", [(configure_trimmed, "f32"), (configure_krum, "f32"), (configure_noise, "f16")],
                         ids=["trimmed", "krum", "noise"])
def test_placement_behind_the_other_modes_and_stages(fa, O, torch_gpu, configure, okind):
    """y is whatever the part's own path leaves (a second aggregator without the reply stage says what), the reply
    stage comes after it; through fa_reduce_parts, where a stage part gets its own launches."""
    part, w = 6, O.weights(D)
    owners = P.Owners(okind)
    with fa.Aggregator(1) as agg, fa.Aggregator(1) as twin:
        for a in (agg, twin):
            configure(fa, a, part)
        agg.set_mx8_reply(True, part)
        for rnd in range(2):
            xs = make_clients(N, "f32", 60 + rnd)
            submit_all(agg, part, xs, w)
            submit_all(twin, part, xs, w)
            want = owners.round(twin.finalize(part))
            agg.reduce_parts([part])
            if rnd == 0:
                R.assert_bits(agg.finalize(part), want[2], "round 1")
            else:
                check_round(agg, part, want, okind, "round 2")


# ------------------------------------------------------------------ layouts

LAYOUTS = {
    "two shards": lambda fa: fa.Aggregator(devices=[0, 0], shared_device=True),
    "three shards": lambda fa: fa.Aggregator(devices=[0, 0, 0], shared_device=True),
    "pieces": lambda fa: fa.Aggregator(1),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_layout_independence(fa, O, torch_gpu, kind, layout):
    """The same bytes on range shards and range pieces as the restatement over the whole bucket (one shard).  Range
    shards are cut at multiples of 64 elements, asserted here through fa_bucket_slot's elem_offset: a block of 32 never
    lies in two GPUs' ranges, so rule 6's exchange cannot arise in a context and is tested on the raw entry
    (test_mx8_reply_gpu.py).  Outlier deltas sit in the blocks on each side of every boundary in turn."""
    part, w = 7, O.weights(D)
    with LAYOUTS[layout](fa) as agg:
        if layout == "pieces":
            agg.set_tuning(piece_span_kib=8, piece_split_kib=-1)
        agg.set_mx8_reply()
        agg.define(part, N, fa_dt(fa, kind), fa_dt(fa, kind), D)
        G = len(agg.devices)
        bounds = [agg.slot(part, g, 0)[2] for g in range(1, G)]
        if layout == "pieces":
            bounds = [off for _, _, off in agg.pieces(part, 0, 0)[1:]]
            assert len(bounds) >= 2
        assert bounds and all(0 < b < N and b % 64 == 0 for b in bounds), bounds
        owners = P.Owners(kind)
        model = None
        for rnd in range(3):
            xs = make_clients(N, kind, 70 + rnd, model)
            if rnd > 0:  # an outlier just below the boundaries in round 2, just above in round 3
                for b in bounds:
                    at = b - 1 if rnd == 1 else b
                    xs[0][at] = R.round_out(np.asarray([R.widen(xs[0][at:at + 1], kind)[0] + 3.0], F32), kind)[0]
            submit_all(agg, part, xs, w)
            want = owners.round(R.round_out(plain_aggregate(O, xs, kind, w), kind))
            if rnd == 0:
                agg.finalize(part)
            else:
                _, e, _ = check_round(agg, part, want, kind, "%s %s round %d" % (kind, layout, rnd + 1))
                for b in bounds:  # the outlier's block has a scale of its own, its neighbour across the boundary not
                    assert e[(b >> 5) - 1] != e[b >> 5]
            model = M.widen(owners.sent, kind)


# ------------------------------------------------------------------ NaN blocks

def test_a_nan_block_is_counted_persists_and_clears(fa, O, torch_gpu):
    part, w = 8, O.weights(D)
    owners = P.Owners("f32")
    with fa.Aggregator(1) as agg:
        agg.define(part, N, fa.F32, fa.F32, D)
        agg.set_mx8_reply(True, part)
        counts = []
        for rnd in range(4):
            xs = make_clients(N, "f32", 80 + rnd)
            if rnd == 1:
                xs[1][100] = np.inf   # block 3
                xs[2][2000] = np.nan  # block 62
            if rnd == 3:  # the owners were sent a clean model by other means
                clean = np.random.default_rng(89).uniform(-1, 1, N).astype(F32)
                agg.set_mx8_reference(part, clean)
                owners.sent = clean.copy()
                R.assert_bits(agg.copy_output(part), clean, "the reference, as a round's output")
            submit_all(agg, part, xs, w)
            want = owners.round(plain_aggregate(O, xs, "f32", w))
            if rnd == 0:
                agg.finalize(part)
                continue
            agg.reduce(part)
            counts.append(agg.mx8_reply_stats(part))  # before anybody fetched the codes
            _, e, out = check_round(agg, part, want, "f32", "round %d" % (rnd + 1))
            assert counts[-1] == int((e == 255).sum()) == agg.mx8_reply_stats(part)
            bad = np.isnan(out)
            assert bad.sum() == 32 * counts[-1] and bad[96:128].all() == (rnd < 3)
        assert counts == [2, 2, 0], counts  # it stays NaN in round 3 although that round's receipts are finite


# ------------------------------------------------------------------ refusals and the part's other entries

def test_refusals_and_defaults(fa, O, torch_gpu):
    n = 67
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as ei:
            agg.set_mx8_reply()
        assert ei.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(ei.value)
        agg.set_mx8_reply(False)  # switching nothing off is fine
    with fa.Aggregator(1, eager=True) as agg:
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)
        with pytest.raises(fa.FaError) as ei:
            agg.set_mx8_reply(True, 1)
        assert ei.value.code == fa.ERR_ARG and "FA_LITERAL" in str(ei.value)
        agg.set_mx8_reply()
        agg.define(2, n, fa.F32, fa.F32, D, mode=fa.LITERAL)  # ignores the context default
        state_error(fa, agg.mx8_reply_stats, 2)
        agg.define(3, n, fa.F32, fa.F32, D)  # takes it: non-eager, never host-side
        w = O.weights(D)
        xs = make_clients(n, "f32", 90)
        pins = []
        for k in range(D):
            p = fa.PinnedBuffer(xs[k].nbytes)
            p.view(F32)[:] = xs[k]
            pins.append(p)
            agg.submit(3, k, p.view(F32), w[k], pinned=True)
            assert agg.progress(3) == (k + 1, 0)
        assert agg.host_read_kept(3) == 0
        R.assert_bits(agg.finalize(3), plain_aggregate(O, xs, "f32", w), "bootstrap")
        for fn in (fa.lib().fa_finalize_mx8, fa.lib().fa_copy_mx8):
            q, e = np.zeros(n, I8), np.zeros(3, U8)
            assert fn(agg.handle, 3, q.ctypes.data, e.ctypes.data, 0x10) == fa.ERR_ARG and "flags" in fa.last_error()
            assert fn(agg.handle, 3, None, e.ctypes.data, 0) == fa.ERR_ARG and "q is null" in fa.last_error()
            assert fn(agg.handle, 99, q.ctypes.data, e.ctypes.data, 0) == fa.ERR_ARG
        # mx8_set_reference is accepted on a part with the reply stage alone
        agg.set_mx8_reference(3, xs[0])
        submit_all(agg, 3, xs, w)
        want = P.reply(plain_aggregate(O, xs, "f32", w), xs[0], "f32")
        check_round(agg, 3, want, "f32", "against a reference set by hand")
        agg.define(4, n, fa.F32, fa.F32, D)
        agg.set_mx8_reply(False, 4)
        with pytest.raises(fa.FaError) as ei:
            agg.set_mx8_reference(4, xs[0])
        assert ei.value.code == fa.ERR_STATE
        del pins
