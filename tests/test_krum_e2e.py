"""End-to-end (GPU): --krum-f through the drop-in aggregator process over loopback TCP.

Five data owners send parts 1, 2 and 3 of the three modules of tests/test_f16_e2e.py; tests/replay_tool replays
the archive files and keeps every reply.  Owner slot 1's archives are the values of a benign owner times 1e3: the
benign owners (0.5 randn) sit about sqrt(n / 2) from each other, the scaled one about 500 sqrt(n) from everyone,
so with --krum-f 1 (m = D - f = 4) its score is about 1e6 times the others' and it alone is left out of every
bucket.  The round line names that owner as left out of every bucket, its scores are those of
tests/krum_ref.py's exact distances to within the sums' n * 2^-53 freedom, every reply is bit-equal to the
helper's aggregate under the reported selection, and every stored CRC-32 equals zlib's.
"""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import krum_ref as K
from conftest import PKG_DIR, ROOT
from test_f16_e2e import _modules, pick_base
from test_server_opt_e2e import _reply_bits

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
REPLAY = os.path.join(ROOT, "tests", "tools", "bin", "fa_replay_owners")
D, F = 5, 1
F32 = np.float32
PARTS = [1, 2, 3]
BOOSTED = 1  # the slot whose archives are scaled by 1e3


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def _write_parts(d, seed0, bf16):
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
                    p.copy_(torch.randn(p.shape).mul_(500.0 if k == BOOSTED else 0.5).to(p.dtype))
            torch.jit.save(torch.jit.script(m), str(d / ("mp%d_owner%d.pt" % (mp, k))))
            flat = torch.cat([p.detach().reshape(-1) for p in ps])
            values.setdefault(mp, []).append(flat.view(torch.int16).numpy().view(np.uint16).copy() if bf16
                                             else flat.numpy().copy())
    return values


def _round(parts_dir, out_dir, flags):
    """One round of the drop-in with `flags` in a process of its own; returns (its round line, its stderr)."""
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "1", "--port-base", str(base)]
                           + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        for line in agg.stderr:  # the owners connect once it listens
            if "listening" in line:
                break
        r = subprocess.run([REPLAY, "--dir", str(parts_dir), "--out", str(out_dir), "-d", str(D), "-c", "1",
                            "--parts", ",".join(map(str, PARTS)), "--port-base", str(base)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["replies"] == len(PARTS) * D
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 0, err[-2000:]
    finally:
        if agg.poll() is None:
            agg.kill()
            agg.wait()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), err


def _one_round(tmp_path, O, bf16):
    kind = "bf16" if bf16 else "f32"
    w = np.full(D, F32(1.0) / F32(D), F32)  # the aggregator's default weights
    parts_dir, out_dir = tmp_path / "parts", tmp_path / "replies"
    parts_dir.mkdir()
    out_dir.mkdir()
    xs = _write_parts(parts_dir, 1300, bf16)
    line, err = _round(parts_dir, out_dir, ["--krum-f", str(F)])
    assert line["krum_f"] == F and line["krum_m"] == D - F
    owners = line["krum_owners"]
    assert len(owners) == D and len(set(owners)) == D
    assert "NO OWNER SELECTED" not in err
    for mp in PARTS:
        assert line["krum_left_out"][str(mp)] == [owners[BOOSTED]], (mp, line["krum_left_out"])
        n = np.asarray(xs[mp][0]).size
        scores = np.asarray([float(s) for s in line["krum_scores"][str(mp)]], np.float64)
        exact = K.scores(K.distances(xs[mp], kind), F)
        assert np.all(np.abs(scores - exact) <= (n + D) * 2.0 ** -53 * exact), (mp, scores, exact)
        assert scores[BOOSTED] > 1e5 * np.delete(scores, BOOSTED).max()
        sel = np.ones(D, bool)
        sel[BOOSTED] = False
        assert K.select(scores, D - F).tolist() == sel.tolist()
        want = K.round_out(K.aggregate(O, xs[mp], kind, w, sel), kind)
        assert np.isfinite(K.widen(want, kind)).all()
        files = sorted(glob.glob(str(out_dir / ("reply_mp%d_port*.pt" % mp))))
        assert len(files) == D
        for f in files:
            K.assert_bits(_reply_bits(f, bf16), want, os.path.basename(f))  # checks the CRC-32s too


def test_the_scaled_owner_is_left_out_of_every_bucket(torch_gpu, O, tmp_path):
    _one_round(tmp_path, O, False)


def test_bf16_archives(torch_gpu, O, tmp_path):
    _one_round(tmp_path, O, True)
