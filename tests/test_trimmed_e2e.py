"""End-to-end (GPU): --mode trimmed / --mode median through the drop-in aggregator process over loopback TCP.

Five data owners send parts 1, 2 and 3 of the three multi-MB modules of tests/test_f16_e2e.py, each owner with
its own seeded fp32 values; owner 3's archives carry NaN in one parameter tensor and 1e30 in another.
tests/replay_tool/replay_owners.cpp replays the archive files and keeps every reply.  Every reply's parameters
are bit-equal to tests/trimmed_ref.py over the five owners (so no NaN and no 1e30 reaches a reply), every stored
CRC-32 equals zlib's over its record, and the round line names the mode and the trim.  One part also goes
through in bf16 (the 16-bit archive path).
"""
import glob
import io
import json
import os
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import trimmed_ref as T
from conftest import PKG_DIR, ROOT
from test_f16_e2e import _modules, pick_base

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
REPLAY = os.path.join(ROOT, "tests", "tools", "bin", "fa_replay_owners")
D = 5
BAD_OWNER = 3


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def _write_parts(d, bf16):
    """DIR/mp<part>_owner<k>.pt and, per part, the owners' flat values as the fp32 the kernel widens them to."""
    import torch
    values = {}
    for k in range(D):
        torch.manual_seed(300 + k)
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
            flat = torch.cat([p.detach().reshape(-1) for p in ps]).float()
            values.setdefault(mp, []).append(flat.numpy().copy())
    return values


@pytest.fixture(scope="module")
def f32_parts(tmp_path_factory):
    d = tmp_path_factory.mktemp("trimmed_parts")
    return d, _write_parts(d, False)


@pytest.fixture(scope="module")
def bf16_parts(tmp_path_factory):
    d = tmp_path_factory.mktemp("trimmed_parts_bf16")
    return d, _write_parts(d, True)


def _reply_bits(path, bf16):
    import torch
    data = open(path, "rb").read()
    zf = zipfile.ZipFile(io.BytesIO(data))
    for info in zf.infolist():  # every stored CRC-32 against zlib over the record
        assert zlib.crc32(zf.read(info.filename)) & 0xFFFFFFFF == info.CRC, info.filename
    ps = list(torch.jit.load(io.BytesIO(data)).parameters())
    assert ps and all(p.dtype == (torch.bfloat16 if bf16 else torch.float32) for p in ps)
    flat = torch.cat([p.detach().reshape(-1) for p in ps])
    return flat.view(torch.int16).numpy().view(np.uint16) if bf16 else flat.numpy().view(np.uint32)


def _round(parts_dir, out_dir, parts, flags):
    """One round of the drop-in with `flags`; returns its round line."""
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "1", "--port-base", str(base)]
                           + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        for line in agg.stderr:  # the owners connect once it listens
            if "listening" in line:
                break
        r = subprocess.run([REPLAY, "--dir", str(parts_dir), "--out", str(out_dir), "-d", str(D), "-c", "1",
                            "--parts", ",".join(map(str, parts)), "--port-base", str(base)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["replies"] == len(parts) * D
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 0, err[-2000:]
    finally:
        if agg.poll() is None:
            agg.kill()
            agg.wait()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _check_replies(out_dir, values, parts, trim, bf16):
    for mp in parts:
        want = T.trimmed(values[mp], trim, out="bf16" if bf16 else "f32")  # values: widened already
        files = sorted(glob.glob(str(out_dir / ("reply_mp%d_port*.pt" % mp))))
        assert len(files) == D
        for f in files:
            got = _reply_bits(f, bf16)
            T.assert_bits(got.view(want.dtype), want, os.path.basename(f))
            assert np.isfinite(T.bf16_to_f32(got) if bf16 else got.view(np.float32)).all()  # nothing of the bad owner's


@pytest.mark.parametrize("flags,trim", [(["--mode", "trimmed", "--trim", "1"], 1), (["--mode", "median"], 2)])
def test_trimmed_round(torch_gpu, f32_parts, tmp_path, flags, trim):
    parts_dir, values = f32_parts
    line = _round(parts_dir, tmp_path, [1, 2, 3], flags)
    assert line["mode"] == "trimmed" and line["trim"] == trim
    _check_replies(tmp_path, values, [1, 2, 3], trim, False)


def test_trimmed_round_bf16_part(torch_gpu, bf16_parts, tmp_path):
    parts_dir, values = bf16_parts
    line = _round(parts_dir, tmp_path, [1, 2, 3], ["--mode", "trimmed", "--trim", "1"])
    assert line["mode"] == "trimmed" and line["trim"] == 1
    _check_replies(tmp_path, values, [1, 2, 3], 1, True)
