"""GPU: the server-optimizer stage (FedAvgM, FedAdagrad, FedAdam, FedYogi) bit for bit against
tests/server_opt_ref.py.

Every comparison covers all elements of x, m, v and the output; where the expected value is NaN only a NaN is
required (random-input cases also assert that the expected values are finite, so that leniency hides nothing).
Parity runs at least three steps after the state is set: a fused beta m + c d agrees with the rule on the
first step after m = v = 0 and differs from the second on (tests/test_server_opt_cpu.py).
"""
import zlib

import numpy as np
import pytest

import server_opt_ref as S
import trimmed_ref as T

pytestmark = pytest.mark.gpu

F16, F32, U16 = np.float16, np.float32, np.uint16
SEED = 0x5E0F
NS = [1, 7, 67, 4099, 100003]
HP = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
KINDS = ["f32", "bf16", "f16"]


def fa_dt(fa, kind):
    return {"f32": fa.F32, "f16": fa.F16, "bf16": fa.BF16}[kind]


def dev_f32(torch, a, offset=0):
    """a (fp32) on the device, `offset` elements into a fresh allocation."""
    t = torch.empty(a.size + 16, dtype=torch.float32, device="cuda")[offset:offset + a.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, F32)))
    return t


def dev_out(torch, n, kind, offset=0):
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind]
    return torch.zeros(n + 16, dtype=dt, device="cuda")[offset:offset + n]


def to_host(torch, t, kind="f32"):
    if kind == "bf16":
        return t.view(torch.int16).cpu().numpy().view(U16)
    return t.cpu().numpy()


def random_state(n, seed):
    """A non-zero state: uniform x, small random m, positive v."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, n).astype(F32), (rng.standard_normal(n) * 0.05).astype(F32),
            rng.uniform(0.01, 1.0, n).astype(F32))


def drifted(x, seed):
    """A fresh aggregate near x: x + N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    return (x + (rng.standard_normal(x.size) * 0.1).astype(F32)).astype(F32)


def check_state(torch, devs, ref, rule, what):
    dx, dm, dv = devs
    T.assert_bits(to_host(torch, dx), ref[0], what + " x")
    T.assert_bits(to_host(torch, dm), ref[1], what + " m")
    if rule != S.MOMENTUM:
        T.assert_bits(to_host(torch, dv), ref[2], what + " v")


def run_steps(fa, torch, rule, okind, n, offsets=(0, 0, 0, 0, 0), steps=3, alias=False, no_out=False, seed=SEED):
    """`steps` consecutive raw steps from an uploaded non-zero state, a fresh aggregate each; every bit of x, m,
    v and out is compared after every step."""
    x, m, v = random_state(n, seed)
    dx, dm = dev_f32(torch, x, offsets[1]), dev_f32(torch, m, offsets[2])
    dv = dev_f32(torch, v, offsets[3]) if rule != S.MOMENTUM else None
    for t in range(steps):
        avg = drifted(x, seed + 1 + t)
        da = dev_f32(torch, avg, offsets[0])
        out = None if no_out else da if alias else dev_out(torch, n, okind, offsets[4])
        fa.server_opt_device(da, dx, dm, dv, n, out, fa_dt(fa, okind), rule=rule, **HP)
        torch.cuda.synchronize()
        x, m, v = S.step(rule, avg, x, m, v, **HP)
        assert np.isfinite(x).all() and np.isfinite(m).all() and (v is None or np.isfinite(v).all())
        what = "%s -> %s n %d step %d offsets %s" % (S.NAMES[rule], okind, n, t + 1, (offsets,))
        check_state(torch, (dx, dm, dv), (x, m, v), rule, what)
        if out is not None:
            T.assert_bits(to_host(torch, out, okind), S.round_out(x, okind), what + " out")


# ------------------------------------------------------------------ raw entry

@pytest.mark.parametrize("okind", KINDS)
@pytest.mark.parametrize("rule", S.RULES)
def test_raw_entry_three_steps(fa, torch_gpu, rule, okind):
    for n in NS:
        run_steps(fa, torch_gpu, rule, okind, n)


@pytest.mark.parametrize("okind", ["f32", "bf16"])
@pytest.mark.parametrize("rule", S.RULES)
def test_raw_entry_pointer_phases(fa, torch_gpu, rule, okind):
    n = 4099
    run_steps(fa, torch_gpu, rule, okind, n, offsets=(1, 1, 1, 1, 1))  # one shared phase: vector body, head and tail
    run_steps(fa, torch_gpu, rule, okind, n, offsets=(0, 1, 2, 3, 0))  # mixed phases: one element per lane
    run_steps(fa, torch_gpu, rule, okind, n, offsets=(2, 2, 2, 2, 3))  # the output's phase alone is off
    run_steps(fa, torch_gpu, rule, okind, 3, offsets=(1, 1, 1, 1, 1))  # shorter than the head


@pytest.mark.parametrize("rule", S.RULES)
def test_raw_entry_in_place_and_states_only(fa, torch_gpu, rule):
    for n in (67, 4099):
        run_steps(fa, torch_gpu, rule, "f32", n, alias=True)      # out is the aggregate's own buffer
        run_steps(fa, torch_gpu, rule, "f32", n, offsets=(3, 3, 3, 3, 3), alias=True)
        run_steps(fa, torch_gpu, rule, "f32", n, no_out=True)     # d_out = NULL


def special_columns(n):
    """(avg, x, m, v) with one column of specials each 16 elements, the rest benign random data."""
    x, m, v = random_state(n, 11)
    avg = drifted(x, 12)
    c = np.arange(n) % 16
    sub = F32(1.4e-45)

    def put(k, a=None, xx=None, mm=None, vv=None):
        for arr, val in ((avg, a), (x, xx), (m, mm), (v, vv)):
            if val is not None:
                arr[c == k] = F32(val)

    put(1, a=np.nan)
    put(2, a=np.inf)
    put(3, a=-np.inf)
    put(4, a=0.0, xx=-0.0, mm=-0.0, vv=0.0)          # d = +0, every product a signed zero
    put(5, a=-0.0, xx=0.0, mm=0.0, vv=-0.0)          # sqrt(-0) = -0
    put(6, a=sub * 3, xx=sub, mm=sub * 5, vv=sub * 7)  # subnormals survive: d = 2 ulp, q underflows to 0
    put(7, a=3.0, xx=1.0, mm=0.0, vv=4.0)            # Yogi: v - q == 0 -> v' = v
    put(8, a=3.0, xx=1.0, mm=0.0, vv=16.0)           # Yogi: v - q > 0
    put(9, a=3.0, xx=1.0, mm=0.0, vv=1.0)            # Yogi: v - q < 0
    put(10, a=3e38, xx=-3e38)                        # d overflows to inf, q = inf
    put(11, a=1e20, xx=0.0, vv=np.inf)               # q = inf, v = inf: Yogi's s is NaN
    put(12, mm=np.nan)
    put(13, vv=np.nan)
    put(14, vv=-1.0)                                 # sqrt of a negative: NaN
    put(15, a=1e-30, xx=0.0, mm=0.0, vv=0.0)         # q and v' subnormal or zero, the step divides by ~tau
    return avg, x, m, v


@pytest.mark.parametrize("okind", KINDS)
@pytest.mark.parametrize("rule", S.RULES)
def test_raw_entry_specials(fa, torch_gpu, rule, okind):
    torch = torch_gpu
    n = 4099
    avg, x, m, v = special_columns(n)
    if okind == "f16":  # x' = x that rounds past 65504 (inf), just below it (65504) and to an fp16 subnormal
        for k, val in ((16, 65520.0), (48, 65519.0), (32, 6e-8)):
            sel = np.arange(n) % 64 == k  # elements of the benign column
            x[sel] = avg[sel] = F32(val)
            m[sel] = F32(0.0)
    hp = dict(lr=1.0, beta1=0.5, beta2=0.75, tau=1.0)
    dx, dm = dev_f32(torch, x), dev_f32(torch, m)
    dv = dev_f32(torch, v) if rule != S.MOMENTUM else None
    for t in range(2):  # the second step runs on the NaNs, infs and zeros the first one left
        da, out = dev_f32(torch, avg), dev_out(torch, n, okind)
        fa.server_opt_device(da, dx, dm, dv, n, out, fa_dt(fa, okind), rule=rule, **hp)
        torch.cuda.synchronize()
        x, m, v1 = S.step(rule, avg, x, m, v, **hp)
        v = v if rule == S.MOMENTUM else v1
        what = "%s specials -> %s step %d" % (S.NAMES[rule], okind, t + 1)
        check_state(torch, (dx, dm, dv), (x, m, v), rule, what)
        T.assert_bits(to_host(torch, out, okind), S.round_out(x, okind), what + " out")


# ------------------------------------------------------------------ through a context, one GPU

def receipts(O, D, n, kind, seed):
    xs = [O.gen(seed, k, n) for k in range(D)]
    if kind == "f16":
        return [x.astype(F16) for x in xs]
    if kind == "bf16":
        return [T.f32_to_bf16(x) for x in xs]
    return xs


def aggregate(O, xs, w, kind):
    """The part's fp32 aggregate: the ordered FMA chain before any rounding."""
    if kind == "bf16":
        return O.fedavg(xs, w, out_dtype="f32")
    return O.fedavg([np.ascontiguousarray(x, F32) if x.dtype == F32 else x.astype(F32) for x in xs], w)


def submit_all(agg, part, xs, w=None):
    for k, x in enumerate(xs):
        agg.submit(part, k, x, 1.0 if w is None else w[k])


def check_part(agg, part, got, ref, rule, okind, steps, what):
    T.assert_bits(got, S.round_out(ref[0], okind), what + " output")
    x, m, v, k = agg.server_opt_state(part)
    assert k == steps, (what, k, steps)
    T.assert_bits(x, ref[0], what + " x")
    T.assert_bits(m, ref[1], what + " m")
    if rule == S.MOMENTUM:
        assert v is None
    else:
        T.assert_bits(v, ref[2], what + " v")


def finite(ref):
    return all(a is None or np.isfinite(a).all() for a in ref)


CTX_CASES = [(D, i, o, S.ADAM) for D in (1, 3, 9) for i, o in (("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("f32", "bf16"))]
CTX_CASES += [(3, "f32", "f32", r) for r in (S.MOMENTUM, S.ADAGRAD, S.YOGI)] + [(3, "f16", "f16", S.MOMENTUM), (9, "bf16", "bf16", S.YOGI)]


@pytest.mark.parametrize("D,ikind,okind,rule", CTX_CASES)
def test_context_bootstrap_then_a_step_by_every_reducing_call(fa, O, torch_gpu, D, ikind, okind, rule):
    n = 4099
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.set_server_opt(rule, **HP)  # the context default: parts defined later take it
        agg.define(1, n, fa_dt(fa, ikind), fa_dt(fa, okind), D)
        # round 1 bootstraps: plain FedAvg's bits, steps 0, the state is (avg, 0, 0)
        xs = receipts(O, D, n, ikind, SEED)
        submit_all(agg, 1, xs, w)
        avg = aggregate(O, xs, w, ikind)
        ref = S.bootstrap(rule, avg)
        check_part(agg, 1, agg.finalize(1), ref, rule, okind, 0, "bootstrap")
        # rounds 2-4: one step each, by finalize / reduce_parts + finalize / reduce + copy_output
        for r, path in enumerate(("finalize", "reduce_parts", "reduce"), start=1):
            xs = receipts(O, D, n, ikind, SEED + r)
            submit_all(agg, 1, xs, w)
            ref = S.step(rule, aggregate(O, xs, w, ikind), ref[0], ref[1], ref[2], **HP)
            assert finite(ref)
            if path == "finalize":
                got = agg.finalize(1)
            elif path == "reduce_parts":
                agg.reduce_parts([1])
                got = agg.finalize(1)  # only copies out: no second step
            else:
                agg.reduce(1)
                got = agg.copy_output(1)
            check_part(agg, 1, got, ref, rule, okind, r, "round %d by %s" % (r + 1, path))
        # reduce marked the round reduced: the finalize after it copies out and takes no step
        check_part(agg, 1, agg.finalize(1), ref, rule, okind, 3, "finalize after reduce")


def test_context_master_set_before_round_one(fa, O, torch_gpu):
    D, n = 3, 4099
    w = O.weights(D)
    x0 = random_state(n, 3)[0]
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        with pytest.raises(fa.FaError) as e:  # no stage yet
            agg.server_opt_state(1)
        assert e.value.code == fa.ERR_STATE
        agg.set_server_opt(S.ADAM, part_id=1, **HP)
        agg.set_server_opt_state(1, x=x0)
        ref = (x0, np.zeros(n, F32), np.zeros(n, F32))
        for r in range(1, 4):  # a real step in round 1: no bootstrap
            xs = receipts(O, D, n, "f32", SEED + r)
            submit_all(agg, 1, xs, w)
            ref = S.step(S.ADAM, aggregate(O, xs, w, "f32"), *ref, **HP)
            assert finite(ref)
            check_part(agg, 1, agg.finalize(1), ref, S.ADAM, "f32", r, "round %d" % r)
        # set m and v alone, with a step count: x stays
        _, m1, v1 = random_state(n, 4)
        agg.set_server_opt_state(1, m=m1, v=v1, steps=40)
        x, m, v, k = agg.server_opt_state(1)
        assert k == 40
        T.assert_bits(x, ref[0], "x kept")
        T.assert_bits(m, m1, "m set")
        T.assert_bits(v, v1, "v set")


def test_context_lr_change_rule_change_and_removal(fa, O, torch_gpu):
    D, n = 3, 4099
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_server_opt(S.ADAM, part_id=1, **HP)

        def round_(seed, rule, ref, hp, steps, what):
            xs = receipts(O, D, n, "f32", seed)
            submit_all(agg, 1, xs, w)
            avg = aggregate(O, xs, w, "f32")
            ref = S.bootstrap(rule, avg) if ref is None else S.step(rule, avg, ref[0], ref[1], ref[2], **hp)
            assert finite(ref)
            check_part(agg, 1, agg.finalize(1), ref, rule, "f32", steps, what)
            return ref

        ref = round_(SEED, S.ADAM, None, HP, 0, "bootstrap")
        ref = round_(SEED + 1, S.ADAM, ref, HP, 1, "step 1")
        ref = round_(SEED + 2, S.ADAM, ref, HP, 2, "step 2")
        # the same rule again: the state stays, the hyperparameters change
        slow = dict(HP, lr=0.025, beta1=0.5)
        agg.set_server_opt(S.ADAM, part_id=1, **slow)
        check_part(agg, 1, agg.copy_output(1), ref, S.ADAM, "f32", 2, "after the lr change")
        ref = round_(SEED + 3, S.ADAM, ref, slow, 3, "step 3 at the new lr")
        # another rule: x stays, m and v are zeroed
        agg.set_server_opt(S.YOGI, part_id=1, **HP)
        ref = (ref[0], np.zeros(n, F32), np.zeros(n, F32))
        x, m, v, k = agg.server_opt_state(1)
        T.assert_bits(x, ref[0], "x kept over the rule change")
        assert not m.any() and not v.any() and k == 3
        for i in range(3):
            ref = round_(SEED + 4 + i, S.YOGI, ref, HP, 4 + i, "yogi step %d" % (i + 1))
        # to momentum: v goes
        agg.set_server_opt(S.MOMENTUM, part_id=1, **HP)
        ref = (ref[0], np.zeros(n, F32), None)
        for i in range(3):
            ref = round_(SEED + 7 + i, S.MOMENTUM, ref, HP, 7 + i, "momentum step %d" % (i + 1))
        # OPT_NONE: plain FedAvg bits again, the state is gone
        agg.set_server_opt(S.NONE, part_id=1)
        xs = receipts(O, D, n, "f32", SEED + 20)
        submit_all(agg, 1, xs, w)
        T.assert_bits(agg.finalize(1), aggregate(O, xs, w, "f32"), "stage removed")
        with pytest.raises(fa.FaError) as e:
            agg.server_opt_state(1)
        assert e.value.code == fa.ERR_STATE


def test_context_every_reduce_is_a_step_and_needs_every_client(fa, O, torch_gpu):
    D, n = 3, 67
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.set_server_opt(S.MOMENTUM, **HP)
        agg.define(1, n, fa.F32, fa.F32, D)
        xs = receipts(O, D, n, "f32", SEED)
        agg.submit(1, 0, xs[0], w[0])
        with pytest.raises(fa.FaError) as e:  # two of three clients are missing
            agg.reduce(1)
        assert e.value.code == fa.ERR_STATE
        agg.submit(1, 1, xs[1], w[1])
        agg.submit(1, 2, xs[2], w[2])
        avg = aggregate(O, xs, w, "f32")
        agg.reduce(1)  # the bootstrap
        ref = S.bootstrap(S.MOMENTUM, avg)
        x0 = random_state(n, 9)[0]
        agg.set_server_opt_state(1, x=x0)
        ref = (x0, ref[1], None)
        for k in range(1, 4):  # a device-resident caller that reduces three times has taken three steps
            agg.reduce(1)
            ref = S.step(S.MOMENTUM, avg, ref[0], ref[1], None, **HP)
            check_part(agg, 1, agg.copy_output(1), ref, S.MOMENTUM, "f32", k, "reduce %d" % k)


def test_rule_change_after_the_reduction_takes_no_second_step(fa, O, torch_gpu):
    D, n = 3, 4099
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.set_server_opt(S.ADAM, **HP)
        assert agg.server_opt()[0] == S.ADAM and agg.server_opt()[1] == F32(HP["lr"])
        agg.define(1, n, fa.F32, fa.F32, D)
        assert agg.server_opt(1)[0] == S.ADAM
        ref = rounds_on(fa, O, agg, D, n, "f32", "f32", S.ADAM, rounds=2, what="before")
        xs = receipts(O, D, n, "f32", SEED + 50)
        submit_all(agg, 1, xs, w)
        agg.reduce_parts([1])  # the round's step
        ref = S.step(S.ADAM, aggregate(O, xs, w, "f32"), *ref, **HP)
        agg.set_server_opt(S.YOGI, part_id=1, **HP)  # x stays, m and v are zeroed; the round stays reduced
        assert agg.server_opt(1)[0] == S.YOGI
        ref = (ref[0], np.zeros(n, F32), np.zeros(n, F32))
        check_part(agg, 1, agg.finalize(1), ref, S.YOGI, "f32", 2, "finalize after the rule change")
        for i in range(3):
            xs = receipts(O, D, n, "f32", SEED + 51 + i)
            submit_all(agg, 1, xs, w)
            ref = S.step(S.YOGI, aggregate(O, xs, w, "f32"), *ref, **HP)
            check_part(agg, 1, agg.finalize(1), ref, S.YOGI, "f32", 3 + i, "yogi step %d" % (i + 1))


def test_stage_removed_on_an_eager_context_leaves_a_plain_part(fa, O, torch_gpu):
    """A part that took the context's stage on an accumulate-on-arrival context was defined without an
    accumulator: with the stage gone it is a plain, non-eager FedAvg part."""
    D, n = 3, 4099
    w = O.weights(D)
    with fa.Aggregator(1, eager=True) as agg:
        agg.set_server_opt(S.ADAM, **HP)
        agg.define(1, n, fa.F32, fa.F32, D)
        rounds_on(fa, O, agg, D, n, "f32", "f32", S.ADAM, rounds=2, what="eager, staged")
        agg.set_server_opt(S.NONE, part_id=1)
        assert agg.server_opt(1)[0] == S.NONE
        for r in range(2):
            xs = receipts(O, D, n, "f32", SEED + 90 + r)
            for k in range(D):
                agg.submit(1, k, xs[k], w[k])
                assert agg.progress(1) == (k + 1, 0)  # nothing is chained on arrival
            T.assert_bits(agg.finalize(1), aggregate(O, xs, w, "f32"), "plain FedAvg after the removal, round %d" % r)
        # a part defined plain on the same context, staged and unstaged again, is eager as before
        agg.set_server_opt(S.NONE)
        agg.define(2, n, fa.F32, fa.F32, D)
        agg.set_server_opt(S.MOMENTUM, part_id=2, **HP)
        agg.set_server_opt(S.NONE, part_id=2)
        xs = receipts(O, D, n, "f32", SEED + 95)
        agg.submit(2, 0, xs[0], w[0])
        agg.submit(2, 1, xs[1], w[1])
        assert agg.progress(2) == (2, 2)
        agg.submit(2, 2, xs[2], w[2])
        T.assert_bits(agg.finalize(2), aggregate(O, xs, w, "f32"), "eager part after a stage came and went")


def test_context_trimmed_mean_feeds_the_stage(fa, O, torch_gpu):
    D, n = 5, 4099
    with fa.Aggregator(1) as agg:
        agg.set_server_opt(S.ADAM, **HP)
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.TRIMMED, trim=1)
        ref = None
        for r in range(4):  # the bootstrap and three steps
            xs = receipts(O, D, n, "f32", SEED + r)
            xs[r % D] = np.full(n, np.nan, F32)  # one owner sends NaN: trimmed away before the stage sees it
            submit_all(agg, 1, xs)
            avg = T.trimmed_f32(xs, 1)
            ref = S.bootstrap(S.ADAM, avg) if ref is None else S.step(S.ADAM, avg, *ref, **HP)
            assert finite(ref)
            check_part(agg, 1, agg.finalize(1), ref, S.ADAM, "f32", r, "trimmed round %d" % (r + 1))


# ------------------------------------------------------------------ layouts

def rounds_on(fa, O, agg, D, n, ikind, okind, rule, x0=None, rounds=3, what="", part=1):
    """`rounds` rounds on a part of agg (the stage already set): the bootstrap first unless x0 gives a master."""
    w = O.weights(D)
    ref = None
    steps = 0
    if x0 is not None:
        agg.set_server_opt_state(part, x=x0)
        ref = (x0, np.zeros(n, F32), None if rule == S.MOMENTUM else np.zeros(n, F32))
    for r in range(rounds):
        xs = receipts(O, D, n, ikind, SEED + 31 * r)
        submit_all(agg, part, xs, w)
        avg = aggregate(O, xs, w, ikind)
        if ref is None:
            ref = S.bootstrap(rule, avg)
        else:
            ref = S.step(rule, avg, ref[0], ref[1], ref[2], **HP)
            steps += 1
        assert finite(ref)
        check_part(agg, part, agg.finalize(part), ref, rule, okind, steps, "%s round %d" % (what, r + 1))
    return ref


def test_three_range_shards_state_crosses_the_boundaries(fa, O, torch_gpu):
    D, n = 3, 100003
    x0, m0, v0 = random_state(n, 21)
    with fa.Aggregator(devices=[0, 0, 0], shared_device=True) as agg:
        agg.set_server_opt(S.YOGI, **HP)
        agg.define(1, n, fa.F32, fa.F32, D)
        agg.set_server_opt_state(1, x=x0, m=m0, v=v0, steps=5)  # scattered to the three shards, gathered back
        x, m, v, k = agg.server_opt_state(1)
        assert k == 5
        T.assert_bits(x, x0, "x round trip")
        T.assert_bits(m, m0, "m round trip")
        T.assert_bits(v, v0, "v round trip")
        agg.set_server_opt_state(1, m=np.zeros(n, F32), v=np.zeros(n, F32), steps=0)
        rounds_on(fa, O, agg, D, n, "f32", "f32", S.YOGI, x0=x0, rounds=3, what="three shards")
    with fa.Aggregator(devices=[0, 0, 0], shared_device=True) as agg:
        agg.set_server_opt(S.ADAM, **HP)
        agg.define(1, n, fa.BF16, fa.BF16, D)  # 16-bit shards over an fp32 master, from the bootstrap
        rounds_on(fa, O, agg, D, n, "bf16", "bf16", S.ADAM, rounds=4, what="three bf16 shards")


@pytest.mark.parametrize("okind", ["f32", "bf16"])
def test_range_pieces(fa, O, torch_gpu, okind):
    D, n = 5, 100003
    with fa.Aggregator(1) as agg:
        agg.set_tuning(piece_span_kib=512, piece_split_kib=-1)  # 5 slots x 128 K elements per piece
        agg.set_server_opt(S.ADAM, **HP)
        agg.define(1, n, fa.F32, fa_dt(fa, okind), D)
        assert len(agg.pieces(1, 0, 0)) >= 3
        rounds_on(fa, O, agg, D, n, "f32", okind, S.ADAM, rounds=4, what="pieces")


def test_refusals_leave_the_context_usable(fa, O, torch_gpu):
    D, n = 3, 67
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        with pytest.raises(fa.FaError) as e:
            agg.set_server_opt(S.ADAM, **HP)
        assert e.value.code == fa.ERR_ARG and "FA_SHARD_CLIENT_RS" in str(e.value)
        agg.define(1, n, fa.F32, fa.F32, D)
        with pytest.raises(fa.FaError) as e:
            agg.set_server_opt(S.ADAM, part_id=1, **HP)
        assert e.value.code == fa.ERR_ARG
    with fa.Aggregator(1) as agg:
        agg.set_server_opt(S.ADAM, **HP)
        agg.define(1, n, fa.F32, fa.F32, D, mode=fa.LITERAL)  # takes no stage from the context
        with pytest.raises(fa.FaError) as e:
            agg.server_opt_state(1)
        assert e.value.code == fa.ERR_STATE
        with pytest.raises(fa.FaError) as e:
            agg.set_server_opt(S.ADAM, part_id=1, **HP)
        assert e.value.code == fa.ERR_ARG and "FA_LITERAL" in str(e.value)
        with pytest.raises(fa.FaError) as e:
            agg.set_server_opt(S.ADAM, lr=0.1, beta1=1.5)
        assert e.value.code == fa.ERR_ARG and "beta1" in str(e.value)
        xs = receipts(O, D, n, "f32", SEED)
        submit_all(agg, 1, xs)
        T.assert_bits(agg.finalize(1), O.literal(xs[-1]), "literal part, untouched")
        agg.define(2, n, fa.F32, fa.F32, D)  # still usable: a FedAvg part takes the context's stage
        rounds_on(fa, O, agg, D, n, "f32", "f32", S.ADAM, rounds=2, what="after refusals", part=2)


def test_crc_host_read_and_eager(fa, O, torch_gpu):
    D, n = 3, 4099
    w = O.weights(D)
    with fa.Aggregator(1) as agg:
        agg.set_server_opt(S.ADAM, **HP)
        agg.define(1, n, fa.F32, fa.F32, D)
        ref = rounds_on(fa, O, agg, D, n, "f32", "f32", S.ADAM, rounds=2, what="crc")
        # the device output after a step: CRC-32 of three byte segments equals zlib's over the copied output
        seg = [4 * 1000, 4 * 99, 4 * 3000]
        raw = agg.copy_output(1).tobytes()
        assert raw == ref[0].tobytes()
        assert agg.output_crc32(1, seg) == [zlib.crc32(raw[sum(seg[:i]):sum(seg[:i + 1])]) for i in range(3)]
        # small pinned receipts, which plain FedAvg would keep host-side: a stage part never does
        xs = receipts(O, D, n, "f32", SEED + 77)
        pins = [fa.PinnedBuffer(n * 4) for _ in range(D)]
        for k in range(D):
            pins[k].view(F32)[:] = xs[k]
            agg.submit(1, k, pins[k].view(F32), w[k], pinned=True)
        assert agg.host_read_kept(1) == 0
        ref = S.step(S.ADAM, aggregate(O, xs, w, "f32"), *ref, **HP)
        outp = fa.PinnedBuffer(n * 4)
        v = outp.view(F32)
        agg.finalize_gather(1, [v[:1000], v[1000:1099], v[1099:]], pinned=True)
        check_part(agg, 1, v.copy(), ref, S.ADAM, "f32", 2, "pinned receipts, gathered reply")
    with fa.Aggregator(1, eager=True) as agg:
        agg.set_server_opt(S.ADAM, **HP)
        agg.define(1, n, fa.F32, fa.F32, D)
        xs = receipts(O, D, n, "f32", SEED)
        submit_all(agg, 1, xs, w)
        assert agg.progress(1) == (D, 0)  # nothing reduced before the finalize
        agg.finalize(1)
        rounds_ref = S.bootstrap(S.ADAM, aggregate(O, xs, w, "f32"))
        for r in range(1, 4):
            xs = receipts(O, D, n, "f32", SEED + r)
            submit_all(agg, 1, xs, w)
            rounds_ref = S.step(S.ADAM, aggregate(O, xs, w, "f32"), *rounds_ref, **HP)
            check_part(agg, 1, agg.finalize(1), rounds_ref, S.ADAM, "f32", r, "eager round %d" % (r + 1))
        # a stage given later to a plain part of an eager context: what it chained so far is dropped, and the
        # part is non-eager from there on
        agg.set_server_opt(S.NONE)  # parts defined from here on: plain
        agg.define(3, n, fa.F32, fa.F32, D)
        agg.submit(3, 0, xs[0], w[0])
        assert agg.progress(3) == (1, 1)  # plain parts of this context still accumulate on arrival
        agg.set_server_opt(S.YOGI, part_id=3, **HP)
        agg.submit(3, 1, xs[1], w[1])
        agg.submit(3, 2, xs[2], w[2])
        assert agg.progress(3) == (D, 0)
        check_part(agg, 3, agg.finalize(3), S.bootstrap(S.YOGI, aggregate(O, xs, w, "f32")), S.YOGI, "f32", 0,
                   "stage set mid-round on an eager context")
