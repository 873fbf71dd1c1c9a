"""End-to-end (GPU): --mode bulyan --bulyan-f through the drop-in aggregator process over loopback TCP.

Seven data owners send parts 1, 2 and 3 of the three modules of tests/test_f16_e2e.py, each with its own seeded
values; owner slot 3's archives carry NaN in one parameter tensor and 1e30 in another, so every distance that
touches it is NaN and with --bulyan-f 1 it is never among the five owners picked.  The round line names the mode,
f and, per bucket, the owners left out: they are those tests/bulyan_ref.py leaves out from the exact distances
(the benign scores differ by parts in a thousand, the sums' freedom is n * 2^-53), every reply is bit-equal to the
helper's centred mean over the reported picks, holds nothing of the bad owner's, and every stored CRC-32 equals
zlib's.
"""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import bulyan_ref as B
from conftest import PKG_DIR, ROOT
from test_f16_e2e import _modules, pick_base
from test_server_opt_e2e import _reply_bits

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
REPLAY = os.path.join(ROOT, "tests", "tools", "bin", "fa_replay_owners")
D, F = 7, 1
PARTS = [1, 2, 3]
BAD_OWNER = 3


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def _write_parts(d, bf16):
    """DIR/mp<part>_owner<k>.pt and, per part, the owners' flat values in the archive's dtype (bf16: the bits)."""
    import torch
    values = {}
    for k in range(D):
        torch.manual_seed(1700 + k)
        for mp, m in _modules().items():
            if bf16:
                m = m.to(torch.bfloat16)
            with torch.no_grad():
                ps = list(m.parameters())
                for p in ps:
                    p.copy_(torch.randn(p.shape).mul_(0.5).to(p.dtype))
                if k == BAD_OWNER:  # a diverged owner: one tensor of NaN, another of 1e30
                    ps[0].fill_(float("nan"))
                    ps[1].fill_(1e30)
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


def _one_round(tmp_path, bf16):
    kind = "bf16" if bf16 else "f32"
    parts_dir, out_dir = tmp_path / "parts", tmp_path / "replies"
    parts_dir.mkdir()
    out_dir.mkdir()
    xs = _write_parts(parts_dir, bf16)
    line, err = _round(parts_dir, out_dir, ["--mode", "bulyan", "--bulyan-f", str(F)])
    assert line["mode"] == "bulyan" and line["bulyan_f"] == F and "trim" not in line
    owners = line["bulyan_owners"]
    assert len(owners) == D and len(set(owners)) == D
    assert "NO OWNER PICKED" not in err
    for mp in PARTS:
        left = line["bulyan_left_out"][str(mp)]
        sel = np.asarray([o not in left for o in owners])
        assert sel.sum() == D - 2 * F and not sel[BAD_OWNER], (mp, left)
        _, _, _, rsel, _ = B.bulyan_round(xs[mp], kind, F)
        assert sel.tolist() == rsel.tolist(), (mp, left)
        want = B.round_out(B.aggregate(xs[mp], kind, sel, F), kind)
        assert np.isfinite(B.widen(want, kind)).all()  # nothing of the bad owner's
        files = sorted(glob.glob(str(out_dir / ("reply_mp%d_port*.pt" % mp))))
        assert len(files) == D
        for f in files:
            B.assert_bits(_reply_bits(f, bf16), want, os.path.basename(f))  # checks the CRC-32s too


def test_the_diverged_owner_is_never_picked(torch_gpu, tmp_path):
    _one_round(tmp_path, False)


def test_bf16_archives(torch_gpu, tmp_path):
    _one_round(tmp_path, True)
