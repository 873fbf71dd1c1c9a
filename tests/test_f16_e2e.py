"""End-to-end (GPU): fp16 model parts through the drop-in aggregator process over loopback TCP.

Three data owners send multi-MB parts saved with ``.half()`` (HalfStorage records), each owner with its own
values; tests/replay_tool/replay_owners.cpp replays the archive files over the wire and keeps every reply.
The replies are loaded here with torch.jit.load: float16 parameters, bit-equal to the fp32 chain over the
owners rounded once to fp16, and every stored CRC-32 equal to zlib's over its record (the records' CRCs come
from the GPU by default -- the path is byte-wise -- and from the host with --crc host).
"""
import glob
import io
import json
import os
import random
import socket
import subprocess
import time
import zipfile
import zlib

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
REPLAY = os.path.join(ROOT, "tests", "tools", "bin", "fa_replay_owners")
D = 3


def pick_base():
    for _ in range(50):
        b = random.randrange(10000, 32000, 100)
        try:
            for p in range(b, b + 40):
                with socket.socket() as s:
                    s.bind(("127.0.0.1", p))
            return b
        except OSError:
            continue
    pytest.fail("no free port range")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def _modules():
    """The three multi-MB parts of tests/test_e2e_aggregator._large_parts."""
    import torch.nn as nn
    return {1: nn.Sequential(nn.Conv2d(3, 64, 3), nn.ReLU(), nn.Conv2d(64, 64, 3)),
            2: nn.Sequential(nn.Linear(1024, 2304), nn.ReLU()),
            3: nn.Sequential(nn.Linear(2304, 1000), nn.ReLU(), nn.Linear(1000, 10))}


@pytest.fixture(scope="module")
def owner_parts(tmp_path_factory, O):
    """DIR/mp<part>_owner<k>.pt in fp16 with each owner's own seeded values, and the expected reply bits."""
    import torch
    d = tmp_path_factory.mktemp("f16_parts")
    values = {}
    for k in range(D):
        torch.manual_seed(100 + k)
        for mp, m in _modules().items():
            m = m.half()
            with torch.no_grad():
                for p in m.parameters():
                    p.copy_(torch.randn(p.shape).mul_(0.5).half())
            torch.jit.save(torch.jit.script(m), str(d / ("mp%d_owner%d.pt" % (mp, k))))
            flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
            values.setdefault(mp, []).append(flat.view(torch.int16).numpy().view(np.float16).copy())
    w = np.full(D, np.float32(1.0) / np.float32(D), np.float32)  # the aggregator's default weights
    expected = {mp: O.fedavg([x.astype(np.float32) for x in xs], w).astype(np.float16)
                for mp, xs in values.items()}
    return d, expected


def _reply_bits(path):
    import torch
    data = open(path, "rb").read()
    zf = zipfile.ZipFile(io.BytesIO(data))
    for info in zf.infolist():  # every stored CRC-32 against zlib over the record
        assert zlib.crc32(zf.read(info.filename)) & 0xFFFFFFFF == info.CRC, info.filename
    m = torch.jit.load(io.BytesIO(data))
    ps = list(m.parameters())
    assert ps and all(p.dtype == torch.float16 for p in ps)
    return torch.cat([p.detach().reshape(-1) for p in ps]).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("extra", [[], ["--crc", "host"]])
def test_f16_parts_one_round(torch_gpu, owner_parts, tmp_path, extra):
    parts_dir, expected = owner_parts
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "1", "--port-base", str(base)]
                           + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        time.sleep(0.5)
        r = subprocess.run([REPLAY, "--dir", str(parts_dir), "--out", str(tmp_path), "-d", str(D), "-c", "1",
                            "--parts", "1,2,3", "--port-base", str(base)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["replies"] == 3 * D
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 0, err[-2000:]
    finally:
        if agg.poll() is None:
            agg.kill()
    for mp, want in expected.items():
        files = sorted(glob.glob(str(tmp_path / ("reply_mp%d_port*.pt" % mp))))
        assert len(files) == D  # one reply per owner (ids 0, 2, 3: aggregator.cpp:102-106 with one compute node)
        for f in files:
            got = _reply_bits(f)
            assert got.size == want.size
            bad = np.flatnonzero(got != want.view(np.uint16))
            assert bad.size == 0, "%s: %d mismatches, first at %s" % (os.path.basename(f), bad.size, bad[:4])


def test_a_bf16_receipt_for_an_f16_bucket_ends_the_process(torch_gpu, owner_parts, tmp_path):
    """Same size, the other 2-byte type: never reduced.  The aggregator exits 1 naming the dtype; no reply."""
    import shutil
    import torch
    parts_dir, _ = owner_parts
    mixed = tmp_path / "parts"
    mixed.mkdir()
    for k in range(D):
        shutil.copy(str(parts_dir / ("mp1_owner%d.pt" % k)), str(mixed / ("mp1_owner%d.pt" % k)))
    torch.manual_seed(7)
    torch.jit.save(torch.jit.script(_modules()[1].to(torch.bfloat16)), str(mixed / "mp1_owner1.pt"))
    out_dir = tmp_path / "replies"
    out_dir.mkdir()
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "1", "--port-base", str(base)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    owners = None
    try:
        time.sleep(0.5)
        owners = subprocess.Popen([REPLAY, "--dir", str(mixed), "--out", str(out_dir), "-d", str(D), "-c", "1",
                                   "--parts", "1", "--port-base", str(base)], stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True)
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 1, (agg.returncode, err[-2000:])
        assert "changed size or dtype" in err
        assert not any(l.startswith("{") for l in out.splitlines())  # no round completed
    finally:
        for p in (agg, owners):
            if p is not None and p.poll() is None:
                p.kill()
                p.wait()
    assert glob.glob(str(out_dir / "*")) == []  # no reply was sent
