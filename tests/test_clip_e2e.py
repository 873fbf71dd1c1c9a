"""End-to-end (GPU): --clip-norm / --clip-state through the drop-in aggregator process over loopback TCP.

Three data owners send parts 1, 2 and 3 of the three modules of tests/test_f16_e2e.py; tests/replay_tool replays
the archive files (one round per process) and keeps every reply.  Round 1 has no stored model: it bootstraps
(plain FedAvg, nothing clipped) and writes the state file.  Round 2 runs in a new aggregator process that reads
the file; owner 1's archives are the values of a benign owner times 1e3, so with C = 5000 it alone is clipped in
every part (the benign owners sit about 0.58 sqrt(n) <= 900 from the stored model, the scaled one at least
1e5).  The squared distances of the round line are within n * 2^-53 * exact of tests/clip_ref.py's exact sums,
every reply is bit-equal to the helper's aggregate under the scales those distances give, every stored CRC-32
equals zlib's, and the state file holds the reply widened to fp32.
"""
import glob
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import clip_ref as R
from conftest import PKG_DIR, ROOT
from test_f16_e2e import _modules
from test_server_opt_e2e import _reply_bits, _round

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
D = 3
F32 = np.float32
PARTS = [1, 2, 3]
C = 5000.0
BOOSTED = 1  # the owner whose round-2 archives are scaled by 1e3


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def _write_parts(d, seed0, bf16, boosted=None):
    """DIR/mp<part>_owner<k>.pt and, per part, the owners' flat values in the archive's dtype (bf16: the bits)."""
    import torch
    values = {}
    for k in range(D):
        torch.manual_seed(seed0 + k)
        for mp, m in _modules().items():
            if bf16:
                m = m.to(torch.bfloat16)
            with torch.no_grad():
                ps = list(m.parameters())
                for p in ps:
                    p.copy_(torch.randn(p.shape).mul_(500.0 if k == boosted else 0.5).to(p.dtype))
            torch.jit.save(torch.jit.script(m), str(d / ("mp%d_owner%d.pt" % (mp, k))))
            flat = torch.cat([p.detach().reshape(-1) for p in ps])
            values.setdefault(mp, []).append(flat.view(torch.int16).numpy().view(np.uint16).copy() if bf16
                                             else flat.numpy().copy())
    return values


def read_clip_state(path):
    data = open(path, "rb").read()
    assert data[:8] == b"FACLIPRF"
    version, n_parts = struct.unpack_from("<II", data, 8)
    assert version == 1
    at, parts = 16, {}
    for _ in range(n_parts):
        pid, pad, n = struct.unpack_from("<iIQ", data, at)
        assert pad == 0
        at += 16
        parts[pid] = np.frombuffer(data, F32, n, at).copy()
        at += 4 * n
    assert at == len(data)
    return parts


def _check_replies(out_dir, want, kind):
    for mp in PARTS:
        files = sorted(glob.glob(str(out_dir / ("reply_mp%d_port*.pt" % mp))))
        assert len(files) == D
        for f in files:
            R.assert_bits(_reply_bits(f, kind == "bf16"), want[mp], os.path.basename(f))  # checks the CRC-32s too


def _two_processes(tmp_path, O, bf16):
    kind = "bf16" if bf16 else "f32"
    w = np.full(D, F32(1.0) / F32(D), F32)  # the aggregator's default weights
    state = tmp_path / "clip.bin"
    flags = ["--clip-norm", str(C), "--clip-state", str(state)]
    dir_a, dir_b = tmp_path / "a", tmp_path / "b"
    dir_a.mkdir()
    dir_b.mkdir()
    xs_a = _write_parts(dir_a, 900, bf16)
    xs_b = _write_parts(dir_b, 950, bf16, boosted=BOOSTED)

    # round 1: no file, so every bucket bootstraps -- plain FedAvg, nothing clipped -- and the file is written
    out1 = tmp_path / "replies1"
    out1.mkdir()
    line = _round(dir_a, out1, flags)
    assert line["clip_norm"] == C and line["clipped"] == 0 and line["excluded"] == 0
    assert all(line["clip_sumsq"][str(mp)] == [0.0] * D for mp in PARTS)
    ones, everyone = np.ones(D, F32), np.ones(D, bool)
    want, g = {}, {}
    for mp in PARTS:
        a = R.aggregate(O, xs_a[mp], kind, w, ones, everyone, np.zeros(xs_a[mp][0].size, F32))
        want[mp] = R.round_out(a, kind)
        g[mp] = R.widen(want[mp], kind)
    _check_replies(out1, want, kind)
    stored = read_clip_state(state)
    assert sorted(stored) == PARTS
    for mp in PARTS:
        R.assert_bits(stored[mp], g[mp], "state file part %d after round 1" % mp)

    # round 2: a new process starts from the file; the boosted owner is scaled down, the others pass
    out2 = tmp_path / "replies2"
    out2.mkdir()
    line = _round(dir_b, out2, flags)
    assert line["clipped"] == len(PARTS) and line["excluded"] == 0
    for mp in PARTS:
        Q = line["clip_sumsq"][str(mp)]
        n = g[mp].size
        for k in range(D):
            exact = R.sumsq(R.widen(xs_b[mp][k], kind), g[mp])
            assert abs(Q[k] - exact) <= R.sumsq_bound(n, exact), (mp, k, Q[k], exact)
        _, scales, included, n_clipped, a = R.clip_round(O, xs_b[mp], kind, w, g[mp], C, Q=Q)
        assert n_clipped == 1 and included.all() and scales[BOOSTED] < 1e-1, (mp, scales)
        want[mp] = R.round_out(a, kind)
        assert np.isfinite(R.widen(want[mp], kind)).all()
    _check_replies(out2, want, kind)
    stored = read_clip_state(state)
    for mp in PARTS:
        R.assert_bits(stored[mp], R.widen(want[mp], kind), "state file part %d after round 2" % mp)
    assert not os.path.exists(str(state) + ".tmp")


def test_two_processes_carry_the_reference_through_the_file(torch_gpu, O, tmp_path):
    _two_processes(tmp_path, O, False)


def test_bf16_archives(torch_gpu, O, tmp_path):
    _two_processes(tmp_path, O, True)
