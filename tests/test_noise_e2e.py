"""End-to-end (GPU): --dp-noise-multiplier / --dp-seed through the drop-in aggregator process over loopback TCP.

Three data owners send parts 1, 2 and 3 as in tests/test_clip_e2e.py (one round per process, --clip-state carries
the model last sent).  With --dp-seed every reply is bit-equal to tests/clip_ref.py's clipped aggregate plus
tests/noise_ref.py's noise of stddev (float)(Z * C * max_k w_k), stream = the part, round 0 of the process; the
round line carries the multiplier, the stddev and the round; the state file holds the noisy reply.  Without
--dp-seed two starts draw different noise.
"""
import os
import subprocess

import numpy as np
import pytest

import clip_ref as R
import noise_ref as N
from conftest import PKG_DIR, ROOT
from test_clip_e2e import BOOSTED, C, D, PARTS, _check_replies, _write_parts, read_clip_state
from test_server_opt_e2e import _reply_bits, _round

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
F32 = np.float32
Z = 1e-4
DP_SEED = 0xD1FFE7E27AA15EED
W = np.full(D, F32(1.0) / F32(D), F32)  # the aggregator's default weights
STDDEV = F32(Z * float(F32(C)) * float(W.max()))


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def _line_ok(line):
    assert line["dp_noise_multiplier"] == Z and F32(line["dp_stddev"]) == STDDEV and line["dp_round"] == 0


@pytest.mark.parametrize("bf16", [False, True])
def test_two_rounds_match_the_references(torch_gpu, O, tmp_path, bf16):
    kind = "bf16" if bf16 else "f32"
    state = tmp_path / "clip.bin"
    flags = ["--clip-norm", str(C), "--clip-state", str(state), "--dp-noise-multiplier", repr(Z), "--dp-seed", hex(DP_SEED)]
    dir_a, dir_b = tmp_path / "a", tmp_path / "b"
    dir_a.mkdir()
    dir_b.mkdir()
    xs_a = _write_parts(dir_a, 900, bf16)
    xs_b = _write_parts(dir_b, 950, bf16, boosted=BOOSTED)

    # round 1: the clip stage bootstraps (nothing clipped); the plain aggregate still gets its noise
    out1 = tmp_path / "replies1"
    out1.mkdir()
    line = _round(dir_a, out1, flags)
    _line_ok(line)
    assert line["clipped"] == 0 and line["excluded"] == 0
    ones, everyone = np.ones(D, F32), np.ones(D, bool)
    want, g = {}, {}
    for mp in PARTS:
        a = R.aggregate(O, xs_a[mp], kind, W, ones, everyone, np.zeros(xs_a[mp][0].size, F32))
        want[mp] = R.round_out(N.noisy(a, STDDEV, DP_SEED, mp, 0), kind)
        assert (want[mp] != R.round_out(a, kind)).mean() > 0.9  # the noise shows in the reply's dtype
        g[mp] = R.widen(want[mp], kind)
    _check_replies(out1, want, kind)
    stored = read_clip_state(state)
    for mp in PARTS:
        R.assert_bits(stored[mp], g[mp], "state file part %d after round 1: the noisy reply" % mp)

    # round 2, a new process: updates are clipped against the noisy model the owners received, then noised
    out2 = tmp_path / "replies2"
    out2.mkdir()
    line = _round(dir_b, out2, flags)
    _line_ok(line)
    assert line["clipped"] == len(PARTS) and line["excluded"] == 0
    for mp in PARTS:
        Q = line["clip_sumsq"][str(mp)]
        for k in range(D):
            exact = R.sumsq(R.widen(xs_b[mp][k], kind), g[mp])
            assert abs(Q[k] - exact) <= R.sumsq_bound(g[mp].size, exact), (mp, k, Q[k], exact)
        _, scales, included, n_clipped, a = R.clip_round(O, xs_b[mp], kind, W, g[mp], C, Q=Q)
        assert n_clipped == 1 and included.all()
        want[mp] = R.round_out(N.noisy(a, STDDEV, DP_SEED, mp, 0), kind)
    _check_replies(out2, want, kind)


def test_without_a_seed_two_starts_differ(torch_gpu, O, tmp_path):
    d = tmp_path / "a"
    d.mkdir()
    xs = _write_parts(d, 900, False)
    replies = []
    for run in range(2):
        out = tmp_path / ("replies%d" % run)
        out.mkdir()
        line = _round(d, out, ["--clip-norm", str(C), "--dp-noise-multiplier", repr(Z)])
        _line_ok(line)
        replies.append({mp: _reply_bits(str(sorted(out.glob("reply_mp%d_port*.pt" % mp))[0]), False) for mp in PARTS})
    for mp in PARTS:
        assert (replies[0][mp] != replies[1][mp]).mean() > 0.9, mp
        noise = replies[0][mp].astype(np.float64) - O.fedavg(xs[mp], W)
        if noise.size >= 1000:  # the stddev asked for, loosely: 5 sigma of the sample deviation's own spread
            assert abs(noise.std() / float(STDDEV) - 1) < 5 / np.sqrt(2 * noise.size), (mp, noise.std())

