"""GPU: the admission rule of libfa's eight stages and the path from the context defaults to a new part, walked as
a whole (csrc/fa_stages.hip).  The expected refusals are written out here from fa.h's text: clip, Krum and geomed
take FA_FEDAVG parts only and at most one of them; Bulyan takes FA_TRIMMED parts only; the server optimizer, noise,
MX8 receipts and MX8 replies take everything but FA_LITERAL.  Whether a part has a stage is asked through the public
entries alone.  The outputs are compared between runs of the library itself, bit for bit: this pins composition, the
parity tests pin the values.  One GPU, range layout, D = 7 (the smallest D that admits Krum and Bulyan with f = 1),
n = 200 (more than one 64-element shard unit, with a tail).
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
N, D, PART = 200, 7, 4
STAGES = ("opt", "clip", "krum", "geomed", "bulyan", "noise", "mx8", "reply")
FAMILY = {"clip": "clip", "krum": "Krum", "geomed": "geomed"}  # measure-then-select: as the messages name them
NAME = {"opt": "server opt", "clip": "clip", "krum": "krum", "geomed": "geomed", "bulyan": "bulyan", "noise": "noise",
        "mx8": "mx8", "reply": "mx8 reply"}
MODE_NAME = ("FA_FEDAVG", "FA_LITERAL", "FA_TRIMMED")  # by fa_mode


def modes_of(fa, s):
    if s in FAMILY:
        return {fa.FEDAVG}
    return {fa.TRIMMED} if s == "bulyan" else {fa.FEDAVG, fa.TRIMMED}


def turn(fa, agg, s, on, part=-1):
    if s == "opt":
        agg.set_server_opt(fa.OPT_ADAM if on else fa.OPT_NONE, lr=0.5, beta1=0.9, beta2=0.99, tau=1e-3, part_id=part)
    elif s == "clip":
        agg.set_clip(0.5 if on else 0.0, part)
    elif s == "krum":
        agg.set_krum(1, None if on else 0, part)
    elif s == "geomed":
        agg.set_geomed(3 if on else 0, 1e-6, None if part < 0 else part)
    elif s == "bulyan":
        agg.set_bulyan(1 if on else None, part)
    elif s == "noise":
        agg.set_noise(0.01 if on else 0.0, 1234, part)
    elif s == "mx8":
        agg.set_mx8(on, part)
    else:
        agg.set_mx8_reply(on, part)


def has(fa, agg, s, part):
    """Whether the part has stage s, by what its getter, its report or fa_submit_mx8 answers."""
    if s == "opt":
        return agg.server_opt(part)[0] != fa.OPT_NONE
    if s == "geomed":
        return agg.geomed(part)[0] != 0
    if s == "noise":
        return agg.noise(part)[0] > 0
    try:
        if s == "mx8":  # a part without a reference refuses a relative receipt either way
            agg.submit_mx8(part, 0, np.zeros(N, np.int8), np.zeros(fa.mx8_scale_bytes(N), np.uint8))
        else:
            {"clip": agg.clip_round, "krum": agg.krum_round, "bulyan": agg.bulyan_round,
             "reply": agg.mx8_reply_stats}[s](part)
    except fa.FaError as e:
        assert e.code == fa.ERR_STATE, str(e)
        return ("does not take MX8 receipts" if s == "mx8" else " has no ") not in str(e)
    return True


def stages_of(fa, agg, part):
    return {s for s in STAGES if has(fa, agg, s, part)}


def refused(fa, fn, cause):
    with pytest.raises(fa.FaError) as ei:
        fn()
    assert ei.value.code == fa.ERR_ARG and cause in str(ei.value), (cause, str(ei.value))


def clients(seed):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, N).astype(F32)
    return [(base + F32(0.05) * rng.standard_normal(N).astype(F32)).astype(F32) for _ in range(D)]


WEIGHTS = (np.arange(1, D + 1) / np.arange(1, D + 1).sum()).astype(F32)


def run_rounds(fa, agg, part, stages=()):
    """Two rounds of the same seeded receipts (the first bootstraps opt, clip and reply; the second has state) ->
    their outputs as bits and, for a reply part, the second round's codes.  An MX8 part's second round takes its first
    receipt as codes against the first round's output."""
    res = []
    for rnd in range(2):
        xs = clients(100 + rnd)
        for k in range(D):
            if rnd == 1 and k == 0 and "mx8" in stages:
                agg.submit_mx8(part, 0, *fa.mx8_encode((xs[0] - res[0]).astype(F32)), weight=WEIGHTS[0])
            else:
                agg.submit(part, k, xs[k], WEIGHTS[k])
        if rnd == 1 and "reply" in stages:
            res.extend(agg.finalize_mx8(part))
            res.append(agg.copy_output(part))
        else:
            res.append(agg.finalize(part))
    return [np.ascontiguousarray(r).view(np.uint8) for r in res]


def same_bits(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, i, np.flatnonzero(x != y)[:8])


@pytest.mark.parametrize("mode", [0, 1, 2], ids=MODE_NAME)
def test_part_level_pairs(fa, torch_gpu, mode):
    """On a fresh part of every mode: set A, then B, for every ordered pair.  Return codes and named causes follow the
    table; after a refusal the part has exactly what it had."""
    with fa.Aggregator(1) as agg:
        for a, b in itertools.product(STAGES, STAGES):
            agg.define(PART, N, fa.F32, fa.F32, D, mode)
            have = set()
            for s in (a, b):
                other = next((t for t in have if t != s and t in FAMILY and s in FAMILY), None)
                if mode not in modes_of(fa, s):
                    refused(fa, lambda: turn(fa, agg, s, True, PART),
                            "%s: part %d is an %s part" % (NAME[s], PART, MODE_NAME[mode]))
                elif other:
                    refused(fa, lambda: turn(fa, agg, s, True, PART),
                            "%s: part %d has a %s stage (the two stages do not compose)" % (NAME[s], PART, FAMILY[other]))
                else:
                    turn(fa, agg, s, True, PART)
                    have.add(s)
                assert stages_of(fa, agg, PART) == have, (a, b, s, MODE_NAME[mode])


def test_default_level_pairs(fa, torch_gpu):
    """Set A as the context default, then B; then one part of each mode has exactly the stages whose modes include it."""
    with fa.Aggregator(1) as agg:
        for a, b in itertools.product(STAGES, STAGES):
            for s in STAGES:
                turn(fa, agg, s, False)
            have = set()
            for s in (a, b):
                other = next((t for t in have if t != s and t in FAMILY and s in FAMILY), None)
                if other:
                    refused(fa, lambda: turn(fa, agg, s, True),
                            "%s: the context default has a %s stage (the two stages do not compose)" % (NAME[s], FAMILY[other]))
                else:
                    turn(fa, agg, s, True)
                    have.add(s)
            assert (agg.server_opt()[0] != fa.OPT_NONE, agg.geomed()[0] != 0, agg.noise()[0] > 0) == \
                   ("opt" in have, "geomed" in have, "noise" in have), (a, b)
            for mode in (fa.FEDAVG, fa.LITERAL, fa.TRIMMED):
                agg.define(PART + mode, N, fa.F32, fa.F32, D, mode)
                assert stages_of(fa, agg, PART + mode) == {s for s in have if mode in modes_of(fa, s)}, (a, b, mode)


def test_refused_define_keeps_the_old_part(fa, torch_gpu):
    """A context default whose D-dependent check fails (Krum with f = 3 at D = 7) refuses the define before the part of
    the same id is touched."""
    with fa.Aggregator(1) as agg:
        agg.define(PART, N, fa.F32, fa.F32, D)
        before = run_rounds(fa, agg, PART)
        agg.set_krum(3)
        refused(fa, lambda: agg.define(PART, N, fa.F32, fa.F32, D), "krum: f = 3 does not fit D = 7 clients")
        assert stages_of(fa, agg, PART) == set()
        same_bits(run_rounds(fa, agg, PART), before, "the old part after the refused define")


@pytest.mark.parametrize("mode", [0, 2], ids=[MODE_NAME[0], MODE_NAME[2]])
def test_order_and_origin_do_not_matter(fa, torch_gpu, mode):
    """Every pair the mode accepts, as A then B on a part, as B then A, and as context defaults before the define:
    both rounds' outputs (and a reply part's codes) are bit-equal across the three."""
    ok = [s for s in STAGES if mode in modes_of(fa, s)]
    with fa.Aggregator(1) as agg:
        for a, b in itertools.combinations(ok, 2):
            if a in FAMILY and b in FAMILY:
                continue
            runs = []
            for order in ((a, b), (b, a)):
                agg.define(PART, N, fa.F32, fa.F32, D, mode)
                for s in order:
                    turn(fa, agg, s, True, PART)
                runs.append(run_rounds(fa, agg, PART, (a, b)))
            for s in (a, b):
                turn(fa, agg, s, True)
            agg.define(PART, N, fa.F32, fa.F32, D, mode)
            for s in (a, b):
                turn(fa, agg, s, False)
            assert stages_of(fa, agg, PART) == {a, b}
            runs.append(run_rounds(fa, agg, PART, (a, b)))
            same_bits(runs[0], runs[1], (a, b, "B then A"))
            same_bits(runs[0], runs[2], (a, b, "as context defaults"))


@pytest.mark.parametrize("mode,stages", [(0, ("opt", "clip", "noise", "mx8", "reply")),
                                         (0, ("opt", "krum", "noise", "mx8", "reply")),
                                         (0, ("opt", "geomed", "noise", "mx8", "reply")),
                                         (2, ("opt", "bulyan", "noise", "mx8", "reply"))])
def test_removal(fa, torch_gpu, mode, stages):
    """Every stage turned off again: the part reports none, and a plain round matches a part that never had one."""
    with fa.Aggregator(1) as agg:
        agg.define(PART, N, fa.F32, fa.F32, D, mode)
        agg.define(PART + 1, N, fa.F32, fa.F32, D, mode)
        for s in stages:
            turn(fa, agg, s, True, PART)
        run_rounds(fa, agg, PART, stages)
        for s in stages:
            turn(fa, agg, s, False, PART)
        assert stages_of(fa, agg, PART) == set()
        same_bits(run_rounds(fa, agg, PART), run_rounds(fa, agg, PART + 1), stages)
