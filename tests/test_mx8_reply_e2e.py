"""End-to-end (GPU): MX8 replies through the drop-in aggregator process (--mx8-reply) over loopback TCP, three rounds.

The owners, parts and rounds of tests/test_mx8_e2e.py: round 1 is full fp32 from all three owners, in round 2 owners 0
and 2 send MX8 archives and owner 1 a full receipt.  Owners 0 and 2 must get MX8 archives back -- their own receipt
archives with the codes and scales of round 2's FedAvg against round 1's reply (tests/mx8_reply_ref.py), every record's
CRC-32 equal to zlib's, loadable with torch.jit.load -- and owner 1 a full archive holding exactly g', the model the
other two hold after adding their reply.  In round 3 every owner sends MX8 against that model: all three replies are MX8
archives and the full reply is never built.
"""
import glob
import io
import json
import os
import re
import shutil
import subprocess
import time
import zipfile
import zlib

import numpy as np
import pytest

import mx8_ref as M
import mx8_reply_ref as P
from test_f16_e2e import pick_base
from test_f16_e2e import _modules
from test_mx8_e2e import AGG, D, OWNERS, built, reply_values, rounds, save_mx8  # noqa: F401  (fixtures, helpers)

pytestmark = pytest.mark.gpu


def load_reply(path):
    """("mx8", q, e) or ("full", values): the reply archive at `path`, every stored CRC-32 checked against zlib's."""
    import torch
    data = open(path, "rb").read()
    zf = zipfile.ZipFile(io.BytesIO(data))
    for info in zf.infolist():
        assert zlib.crc32(zf.read(info.filename)) & 0xFFFFFFFF == info.CRC, (path, info.filename)
    m = torch.jit.load(io.BytesIO(data))
    ps = list(m.parameters())
    if len(ps) == 1 and ps[0].dtype == torch.int8:
        bs = list(m.buffers())
        assert len(bs) == 1 and bs[0].dtype == torch.uint8
        return "mx8", ps[0].detach().numpy(), bs[0].numpy()
    return "full", reply_values(path)


@pytest.fixture(scope="module")
def three_rounds(rounds, tmp_path_factory, O):
    """The two rounds of test_mx8_e2e and a third in which every owner sends MX8 against g', the model round 2's
    replies left with them; (dir, expect1, expect2, round 3's (q, e) per part)."""
    src, expect1, expect2, _ = rounds
    d = tmp_path_factory.mktemp("mx8_reply_rounds")
    for r in ("r1", "r2"):
        shutil.copytree(str(src / r), str(d / r))
    (d / "r3").mkdir()
    rng = np.random.default_rng(0x3E2F)
    w = np.full(D, np.float32(1.0) / np.float32(D), np.float32)
    expect3 = {}
    for mp in _modules():
        g = P.reply(expect2[mp], expect1[mp], "f32")[2]
        xs = []
        for k in range(D):
            x = (g + np.float32(0.01) * rng.standard_normal(g.size).astype(np.float32)).astype(np.float32)
            q, e = M.encode((x - g).astype(np.float32))
            save_mx8(d / "r3" / ("mp%d_owner%d.pt" % (mp, k)), q, e)
            xs.append(M.expand(q, e, 0, "f32", g, "f32"))
        expect3[mp] = P.reply(O.fedavg(xs, w), g, "f32")[:2]
    return d, expect1, expect2, expect3


def test_mixed_round_gets_mixed_replies(torch_gpu, three_rounds, tmp_path):
    parts_dir, expect1, expect2, expect3 = three_rounds
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "3", "--port-base", str(base),
                            "--mx8-reply"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        time.sleep(0.5)
        r = subprocess.run([OWNERS, "--dir", str(parts_dir), "--out", str(tmp_path), "-d", str(D), "-c", "1",
                            "--parts", "1,2,3", "--rounds", "3", "--port-base", str(base)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["replies"] == 3 * 3 * D
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 0, err[-2000:]
    finally:
        if agg.poll() is None:
            agg.kill()
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert [l["round"] for l in lines] == [0, 1, 2]
    assert (lines[0]["mx8_replies"], lines[0]["mx8_bytes_out"], lines[0]["mx8_nan_blocks"]) == (0, 0, 0)
    assert lines[1]["mx8_receipts"] == 6
    # round 1: the bootstrap, full replies to everyone, holding the plain FedAvg
    for mp, want in expect1.items():
        files = sorted(glob.glob(str(tmp_path / ("r1_reply_mp%d_port*.pt" % mp))))
        assert len(files) == D
        for f in files:
            M.assert_bits(reply_values(f), want, "round 1 %s" % os.path.basename(f))
    # round 2: owner 0 listens alone on its port, owners 1 and 2 share one
    bytes_out = full_bytes = 0
    for mp, y in expect2.items():
        q, e, g = P.reply(y, expect1[mp], "f32")
        assert np.abs(q).max() > 64 and not np.array_equal(g.view(np.uint32), y.view(np.uint32))  # real codes, lossy
        by_port = {}
        for f in glob.glob(str(tmp_path / ("r2_reply_mp%d_port*.pt" % mp))):
            by_port.setdefault(int(re.search(r"_port(\d+)_", f).group(1)), []).append(f)
        assert sorted(len(v) for v in by_port.values()) == [1, 2], by_port
        kinds = {}
        for port, files in by_port.items():
            for f in files:
                rep = load_reply(f)
                kinds.setdefault(len(files), []).append(rep[0])
                what = "round 2 part %d %s" % (mp, os.path.basename(f))
                if rep[0] == "mx8":
                    assert np.array_equal(rep[2], e), what
                    assert np.array_equal(rep[1], q), (what, np.flatnonzero(rep[1] != q)[:8])
                    bytes_out += os.path.getsize(f)
                else:
                    M.assert_bits(rep[1], g, what)  # the model the MX8 owners hold, not the aggregate
                    full_bytes += os.path.getsize(f)
        assert kinds[1] == ["mx8"] and sorted(kinds[2]) == ["full", "mx8"], kinds
        # an MX8 reply is the owner's own receipt archive, record for record
        for k in (0, 2):
            assert os.path.getsize(str(parts_dir / "r2" / ("mp%d_owner%d.pt" % (mp, k)))) in [
                os.path.getsize(f) for fs in by_port.values() for f in fs]
    assert (lines[1]["mx8_replies"], lines[1]["mx8_bytes_out"], lines[1]["mx8_nan_blocks"]) == (6, bytes_out, 0)
    # round 3: MX8 from everyone, MX8 to everyone
    bytes3 = 0
    for mp, (q, e) in expect3.items():
        files = glob.glob(str(tmp_path / ("r3_reply_mp%d_port*.pt" % mp)))
        assert len(files) == D
        for f in files:
            rep = load_reply(f)
            assert rep[0] == "mx8" and np.array_equal(rep[2], e) and np.array_equal(rep[1], q), os.path.basename(f)
            bytes3 += os.path.getsize(f)
    assert (lines[2]["mx8_receipts"], lines[2]["mx8_replies"], lines[2]["mx8_bytes_out"]) == (9, 9, bytes3)
    print("reply bytes of round 2: %d in 6 MX8 archives, %d in 3 full ones: %.2fx smaller per owner"
          % (bytes_out, full_bytes, (full_bytes / 3) / (bytes_out / 6)))


def test_mx8_reply_flag_refusals():
    """--mx8-reply implies --mx8 and is refused where that is: the usage and exit 2, before a device or a socket."""
    for extra in (["--mode", "literal"], ["--layout", "rs"]):
        r = subprocess.run([AGG, "-i", "-1", "-d", "3", "-c", "1", "--mx8-reply"] + extra, capture_output=True, text=True,
                           timeout=30)
        assert r.returncode == 2 and "--mx8-reply" in r.stderr and "usage:" in r.stderr, (extra, r.stderr[-500:])
