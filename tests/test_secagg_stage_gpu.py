"""GPU: the secagg stage through Aggregator (fa.h "Secagg stage") -- a simulated protocol round with a dropout against
the survivors' plain codes, range shards, the stages behind it, the per-round terms and the admission rule.
"""
import numpy as np
import pytest

import noise_ref as N
import server_opt_ref as S

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
N_ELEMS, OWNERS, DROPPED, Q = 3000, 5, 3, 65536.0
SURVIVORS = [k for k in range(OWNERS) if k != DROPPED]
PART, SEED = 3, 0x5EC0DE


@pytest.fixture(scope="module")
def protocol_round(fa):
    """(the survivors' masked buckets, the server's terms, the expected aggregate): every owner masks its fixed-point
    update with a self mask and one pairwise mask per other owner (+ towards a higher id, - towards a lower one);
    owner 3 drops after the others have masked against it.  The expectation holds no ChaCha20: the survivors' plain
    codes summed as Python integers, wrapped to int32, decoded."""
    rng = np.random.default_rng(5)
    words = lambda k: rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(U32)
    nonce = words(3)
    self_key = [words(8) for _ in range(OWNERS)]
    pair_key = {(i, j): words(8) for i in range(OWNERS) for j in range(i + 1, OWNERS)}
    codes = [fa.secagg_quantize(rng.normal(0, 0.3, N_ELEMS).astype(F32), Q)[0] for _ in range(OWNERS)]
    ys = []
    for k in SURVIVORS:
        y = codes[k].view(U32) + fa.secagg_mask_host(self_key[k], nonce, 0, N_ELEMS)
        for (i, j), key in pair_key.items():
            if k in (i, j):
                m = fa.secagg_mask_host(key, nonce, 0, N_ELEMS)
                y = y + m if k == i else y - m
        ys.append(y)
    # the server cancels the survivors' self masks, and the pairwise masks the dropped owner never cancelled
    terms = [(self_key[k], -1) for k in SURVIVORS]
    terms += [(pair_key[min(k, DROPPED), max(k, DROPPED)], -1 if k < DROPPED else 1) for k in SURVIVORS]
    keys, signs = np.stack([t[0] for t in terms]), [t[1] for t in terms]
    total = [sum(int(codes[k][i]) for k in SURVIVORS) for i in range(N_ELEMS)]
    wrapped = np.asarray([(t + 2 ** 31) % 2 ** 32 - 2 ** 31 for t in total], np.int64).astype(np.int32)
    want = (wrapped.astype(F32) * F32(1 / Q)).astype(F32)
    return ys, (keys, np.tile(nonce, (len(terms), 1)), signs), want


def run_round(agg, ys, terms):
    agg.secagg_terms(PART, *terms)
    for slot, y in enumerate(ys):
        agg.submit(PART, slot, y)
    return agg.finalize(PART)


@pytest.mark.parametrize("shards", [1, 2])
def test_protocol_round_with_a_dropout(fa, torch_gpu, protocol_round, shards):
    ys, terms, want = protocol_round
    with fa.Aggregator(devices=[0] * shards, shared_device=shards > 1) as agg:
        agg.define(PART, N_ELEMS, fa.F32, fa.F32, len(ys))
        agg.set_secagg(1 / Q, PART)
        got = run_round(agg, ys, terms)
        assert agg.host_read_kept(PART) == 0
        assert np.array_equal(got.view(U32), want.view(U32))
        # terms are per round: the next reducing call has none until they are set again
        for slot, y in enumerate(ys):
            agg.submit(PART, slot, y)
        with pytest.raises(fa.FaError) as e:
            agg.reduce(PART)
        assert e.value.code == fa.ERR_STATE and "terms" in str(e.value)
        assert np.array_equal(run_round(agg, ys, terms).view(U32), want.view(U32))


def test_noise_and_fedadam_behind_the_stage(fa, torch_gpu, protocol_round):
    ys, terms, want = protocol_round
    hp = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
    x0 = np.random.default_rng(9).uniform(-1, 1, N_ELEMS).astype(F32)
    with fa.Aggregator(1) as agg:
        agg.define(PART, N_ELEMS, fa.F32, fa.BF16, len(ys))
        agg.set_secagg(1 / Q, PART)
        agg.set_noise(0.01, SEED, PART)
        agg.set_server_opt(S.ADAM, part_id=PART, **hp)
        agg.set_server_opt_state(PART, x=x0)
        out = run_round(agg, ys, terms)
        x1, m1, v1 = S.step(S.ADAM, N.noisy(want, 0.01, SEED, PART, 0), x0, np.zeros(N_ELEMS, F32), np.zeros(N_ELEMS, F32), **hp)
        x, m, v, steps = agg.server_opt_state(PART)
        assert steps == 1
        for got, exp in ((x, x1), (m, m1), (v, v1)):
            assert np.array_equal(got.view(U32), exp.view(U32))
        assert np.array_equal(out, S.round_out(x1, "bf16"))


def test_admission(fa, torch_gpu):
    def refused(call, word):
        with pytest.raises(fa.FaError) as e:
            call()
        assert e.value.code == fa.ERR_ARG and word in str(e.value), str(e.value)

    with fa.Aggregator(1) as agg:
        agg.define(1, 256, fa.BF16, fa.BF16, 3)
        refused(lambda: agg.set_secagg(1.0, 1), "bf16 slots")
        agg.define(2, 256, fa.F32, fa.F32, 3, fa.TRIMMED)
        refused(lambda: agg.set_secagg(1.0, 2), "FA_TRIMMED")
        refused(lambda: agg.set_secagg(1.0, -1), "context default")
        for name, setter in (("clip", lambda p: agg.set_clip(1.0, p)), ("Krum", lambda p: agg.set_krum(0, None, p)),
                             ("geomed", lambda p: agg.set_geomed(2, part=p)), ("MX8", lambda p: agg.set_mx8(True, p))):
            agg.define(4, 256, fa.F32, fa.F32, 3)
            setter(4)
            refused(lambda: agg.set_secagg(1.0, 4), name + " stage")
            agg.define(5, 256, fa.F32, fa.F32, 3)
            agg.set_secagg(1.0, 5)
            refused(lambda: setter(5), "secagg stage")
        agg.set_secagg(0.0, 5)  # off again: the part takes the other stages
        agg.set_clip(1.0, 5)
        with pytest.raises(fa.FaError) as e:
            agg.secagg_terms(5, [], [], [])
        assert e.value.code == fa.ERR_STATE
    with fa.Aggregator(devices=[0, 0], rs=True, shared_device=True) as agg:
        agg.define(1, 256, fa.F32, fa.F32, 3)
        refused(lambda: agg.set_secagg(1.0, 1), "FA_SHARD_CLIENT_RS")
