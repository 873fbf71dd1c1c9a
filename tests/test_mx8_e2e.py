"""End-to-end (GPU): MX8 receipts through the drop-in aggregator process (--mx8) over loopback TCP, two rounds.

Three data owners and the three multi-MB parts of tests/test_f16_e2e.  Round 1 is full fp32 from everyone; its
reply is the oracle's FedAvg, so round 2 can be written before any process starts: owners 0 and 2 send their update
against that reply as MX8 archives (one int8 parameter, one uint8 buffer), owner 1 a full receipt.
tests/mx8_tool/mx8_owners.cpp replays the files and keeps every reply.  Every round-2 reply must be the chain over
[g + d_0, x_1, g + d_2], bit for bit, fp32, with every stored CRC-32 equal to zlib's.
"""
import glob
import io
import json
import os
import subprocess
import time
import zipfile
import zlib

import numpy as np
import pytest

import mx8_ref as M
from conftest import PKG_DIR, ROOT
from test_f16_e2e import _modules, pick_base

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
OWNERS = os.path.join(ROOT, "tests", "tools", "bin", "fa_mx8_owners")
D = 3
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "mx8_tool"), OWNERS], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def save_full(path, module, flat):
    """`module` with its parameters set to the fp32 values `flat` (named_parameters order), scripted and saved."""
    import torch
    at = 0
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.from_numpy(flat[at:at + p.numel()].reshape(tuple(p.shape))))
            at += p.numel()
    assert at == flat.size
    torch.jit.save(torch.jit.script(module), str(path))


def save_mx8(path, q, e):
    """The owner's side of the wire format: one int8 parameter, one uint8 buffer."""
    import torch
    import torch.nn as nn

    class Mx8Update(nn.Module):
        def __init__(self):
            super().__init__()
            self.q = nn.Parameter(torch.from_numpy(q), requires_grad=False)
            self.register_buffer("e", torch.from_numpy(e))

        def forward(self, x):
            return x

    torch.jit.save(torch.jit.script(Mx8Update()), str(path))


@pytest.fixture(scope="module")
def rounds(tmp_path_factory, O):
    """DIR/r1 and DIR/r2 as fa_mx8_owners reads them, and the expected reply values of both rounds."""
    d = tmp_path_factory.mktemp("mx8_rounds")
    (d / "r1").mkdir()
    (d / "r2").mkdir()
    rng = np.random.default_rng(0x3E2E)
    w = np.full(D, F32(1.0) / F32(D), F32)  # the aggregator's default weights
    expect1, expect2, mx8_bytes = {}, {}, 0
    for mp in _modules():
        n = sum(p.numel() for p in _modules()[mp].parameters())
        xs1 = [(0.5 * rng.standard_normal(n)).astype(F32) for _ in range(D)]
        for k in range(D):
            save_full(d / "r1" / ("mp%d_owner%d.pt" % (mp, k)), _modules()[mp], xs1[k])
        g = O.fedavg(xs1, w)
        expect1[mp] = g
        xs2 = []
        for k in range(D):
            x = (g + F32(0.01) * rng.standard_normal(n).astype(F32)).astype(F32)  # one local step away from g
            path = d / "r2" / ("mp%d_owner%d.pt" % (mp, k))
            if k == 1:
                save_full(path, _modules()[mp], x)
                xs2.append(x)
            else:
                q, e = M.encode((x - g).astype(F32))  # delta = fl32(x - g), then the encoder
                save_mx8(path, q, e)
                xs2.append(M.expand(q, e, 0, "f32", g, "f32"))
                mx8_bytes += os.path.getsize(str(path))
        expect2[mp] = O.fedavg(xs2, w)
    return d, expect1, expect2, mx8_bytes


def reply_values(path):
    import torch
    data = open(path, "rb").read()
    zf = zipfile.ZipFile(io.BytesIO(data))
    for info in zf.infolist():  # every stored CRC-32 against zlib over the record
        assert zlib.crc32(zf.read(info.filename)) & 0xFFFFFFFF == info.CRC, info.filename
    m = torch.jit.load(io.BytesIO(data))
    ps = list(m.parameters())
    assert ps and all(p.dtype == torch.float32 for p in ps)
    return torch.cat([p.detach().reshape(-1) for p in ps]).numpy()


def test_two_rounds_full_then_mixed(torch_gpu, rounds, tmp_path):
    parts_dir, expect1, expect2, mx8_bytes = rounds
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "2", "--port-base", str(base), "--mx8"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        time.sleep(0.5)
        r = subprocess.run([OWNERS, "--dir", str(parts_dir), "--out", str(tmp_path), "-d", str(D), "-c", "1",
                            "--parts", "1,2,3", "--rounds", "2", "--port-base", str(base)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["replies"] == 2 * 3 * D
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 0, err[-2000:]
    finally:
        if agg.poll() is None:
            agg.kill()
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert [l["round"] for l in lines] == [0, 1]
    assert (lines[0]["mx8_receipts"], lines[0]["mx8_bytes_in"]) == (0, 0)
    assert (lines[1]["mx8_receipts"], lines[1]["mx8_bytes_in"]) == (6, mx8_bytes)
    for rnd, expected in ((1, expect1), (2, expect2)):
        for mp, want in expected.items():
            files = sorted(glob.glob(str(tmp_path / ("r%d_reply_mp%d_port*.pt" % (rnd, mp)))))
            assert len(files) == D  # one reply per owner
            for f in files:
                M.assert_bits(reply_values(f), want, "round %d %s" % (rnd, os.path.basename(f)))


@pytest.mark.parametrize("flag,message", [(["--mx8"], "MX8 receipt for part 1 from owner 0"),
                                          ([], "parameters not all fp32, bf16 or fp16")])
def test_an_mx8_receipt_in_round_one_ends_the_process(torch_gpu, rounds, tmp_path, flag, message):
    """No round reduced, no bucket defined: with --mx8 exit 1 naming the part and the owner; without it the receipt
    ends the process as any archive of another parameter type does.  No reply either way."""
    import shutil
    parts_dir, _, _, _ = rounds
    first = tmp_path / "parts" / "r1"
    first.mkdir(parents=True)
    shutil.copy(str(parts_dir / "r2" / "mp1_owner0.pt"), str(first / "mp1_owner0.pt"))  # the MX8 one, sent first
    for k in (1, 2):
        shutil.copy(str(parts_dir / "r1" / ("mp1_owner%d.pt" % k)), str(first / ("mp1_owner%d.pt" % k)))
    out_dir = tmp_path / "replies"
    out_dir.mkdir()
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "1", "--port-base", str(base)] + flag,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    owners = None
    try:
        time.sleep(0.5)
        owners = subprocess.Popen([OWNERS, "--dir", str(tmp_path / "parts"), "--out", str(out_dir), "-d", str(D), "-c", "1",
                                   "--parts", "1", "--rounds", "1", "--port-base", str(base)], stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True)
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 1, (agg.returncode, err[-2000:])
        assert message in err, err[-2000:]
        assert not any(l.startswith("{") for l in out.splitlines())  # no round completed
    finally:
        for p in (agg, owners):
            if p is not None and p.poll() is None:
                p.kill()
                p.wait()
    assert glob.glob(str(out_dir / "*")) == []  # no reply was sent


def test_mx8_flag_refusals():
    """--mx8 with --mode literal or --layout rs: the usage and exit 2, before a device or a socket is opened."""
    for extra in (["--mode", "literal"], ["--layout", "rs"]):
        r = subprocess.run([AGG, "-i", "-1", "-d", "3", "-c", "1", "--mx8"] + extra, capture_output=True, text=True,
                           timeout=30)
        assert r.returncode == 2 and "--mx8" in r.stderr and "usage:" in r.stderr, (extra, r.stderr[-500:])
