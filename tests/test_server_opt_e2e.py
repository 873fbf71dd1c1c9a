"""End-to-end (GPU): --server-opt through the drop-in aggregator process over loopback TCP.

Three data owners send parts 1, 2 and 3 of the three multi-MB modules of tests/test_f16_e2e.py, each owner with
its own seeded values; tests/replay_tool/replay_owners.cpp replays the archive files (one round per process) and
keeps every reply.  The global model and the moments travel from one aggregator process to the next through
--server-state: every reply's parameters and the state file are bit-equal to tests/server_opt_ref.py over the
fp32 FedAvg chain of the owners, every stored CRC-32 equals zlib's over its record, and the round line names the
rule, the rate and the steps taken.
"""
import glob
import io
import json
import os
import struct
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import server_opt_ref as S
from conftest import PKG_DIR, ROOT
from test_f16_e2e import _modules, pick_base

pytestmark = pytest.mark.gpu

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
REPLAY = os.path.join(ROOT, "tests", "tools", "bin", "fa_replay_owners")
D = 3
F32 = np.float32
PARTS = [1, 2, 3]
LR = 0.1
HP = dict(lr=LR, beta1=0.9, beta2=0.99, tau=1e-3)  # the drop-in's defaults
FLAGS = ["--server-opt", "adam", "--server-lr", "0.1"]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR


def _write_parts(d, seed0, bf16):
    """DIR/mp<part>_owner<k>.pt and, per part, the owners' flat values as the fp32 the kernel widens them to."""
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
                    p.copy_(torch.randn(p.shape).mul_(0.5).to(p.dtype))
            torch.jit.save(torch.jit.script(m), str(d / ("mp%d_owner%d.pt" % (mp, k))))
            values.setdefault(mp, []).append(torch.cat([p.detach().reshape(-1) for p in ps]).float().numpy().copy())
    return values


@pytest.fixture(scope="module")
def sets(tmp_path_factory, O):
    """Archive sets A and B (other seeds) in fp32 and bf16: (directory, the part's fp32 aggregate) each."""
    w = np.full(D, F32(1.0) / F32(D), F32)  # the aggregator's default weights
    out = {}
    for name, seed0, bf16 in (("A", 500, False), ("B", 600, False), ("A16", 700, True), ("B16", 800, True)):
        d = tmp_path_factory.mktemp("server_opt_parts_" + name)
        values = _write_parts(d, seed0, bf16)
        out[name] = (d, {mp: O.fedavg(xs, w) for mp, xs in values.items()})
    return out


def write_state(path, rule, parts):
    """parts: {part id: (x, m, v, steps)}."""
    with open(path, "wb") as f:
        f.write(b"FASRVOPT" + struct.pack("<IIII", 1, rule, len(parts), 0))
        for pid in sorted(parts):
            x, m, v, steps = parts[pid]
            f.write(struct.pack("<iIQQ", pid, 0, x.size, steps))
            for a in (x, m, v):
                f.write(np.ascontiguousarray(a, F32).tobytes())


def read_state(path):
    data = open(path, "rb").read()
    assert data[:8] == b"FASRVOPT"
    version, rule, n_parts, zero = struct.unpack_from("<IIII", data, 8)
    assert (version, zero) == (1, 0)
    at, parts = 24, {}
    for _ in range(n_parts):
        pid, pad, n, steps = struct.unpack_from("<iIQQ", data, at)
        assert pad == 0
        at += 24
        arrs = [np.frombuffer(data, F32, n, at + 4 * n * i).copy() for i in range(3)]
        at += 12 * n
        parts[pid] = (arrs[0], arrs[1], arrs[2], steps)
    assert at == len(data)
    return rule, parts


def _reply_bits(path, bf16):
    import torch
    data = open(path, "rb").read()
    zf = zipfile.ZipFile(io.BytesIO(data))
    for info in zf.infolist():  # every stored CRC-32 against zlib over the record
        assert zlib.crc32(zf.read(info.filename)) & 0xFFFFFFFF == info.CRC, info.filename
    ps = list(torch.jit.load(io.BytesIO(data)).parameters())
    assert ps and all(p.dtype == (torch.bfloat16 if bf16 else torch.float32) for p in ps)
    flat = torch.cat([p.detach().reshape(-1) for p in ps])
    return flat.view(torch.int16).numpy().view(np.uint16) if bf16 else flat.numpy()


def _round(parts_dir, out_dir, flags):
    """One round of the drop-in with `flags` in a process of its own; returns its round line."""
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
    return json.loads(lines[0])


def _check_replies(out_dir, want, bf16):
    """want: {part: fp32 x'}; every owner's reply holds it in the archive's dtype."""
    for mp in PARTS:
        files = sorted(glob.glob(str(out_dir / ("reply_mp%d_port*.pt" % mp))))
        assert len(files) == D
        ref = S.round_out(want[mp], "bf16" if bf16 else "f32")
        for f in files:
            S.assert_bits(_reply_bits(f, bf16), ref, os.path.basename(f))


def _check_state(path, want, steps):
    """want: {part: (x, m, v)}."""
    rule, parts = read_state(path)
    assert rule == S.ADAM and sorted(parts) == PARTS
    for mp in PARTS:
        x, m, v, k = parts[mp]
        assert k == steps
        for got, ref, name in zip((x, m, v), want[mp], "xmv"):
            S.assert_bits(got, ref, "state file part %d %s" % (mp, name))
    assert not os.path.exists(str(path) + ".tmp")


def _line_ok(line, steps):
    assert line["server_opt"] == "adam" and line["server_lr"] == LR and line["server_steps"] == steps


def _two_processes(sets, tmp_path, a, b, bf16):
    dir_a, avg_a = sets[a]
    dir_b, avg_b = sets[b]
    state = tmp_path / "state.bin"
    rng = np.random.default_rng(42)
    ref = {}
    for mp in PARTS:
        n = avg_a[mp].size
        ref[mp] = (rng.uniform(-1, 1, n).astype(F32), np.zeros(n, F32), np.zeros(n, F32))
    write_state(state, S.ADAM, {mp: ref[mp] + (0,) for mp in PARTS})
    for step, (parts_dir, avg) in enumerate(((dir_a, avg_a), (dir_b, avg_b)), start=1):
        out_dir = tmp_path / ("replies%d" % step)
        out_dir.mkdir()
        line = _round(parts_dir, out_dir, FLAGS + ["--server-state", str(state)])
        ref = {mp: S.step(S.ADAM, avg[mp], *ref[mp], **HP) for mp in PARTS}
        assert all(np.isfinite(a_).all() for mp in PARTS for a_ in ref[mp])
        _line_ok(line, step)
        _check_replies(out_dir, {mp: ref[mp][0] for mp in PARTS}, bf16)
        _check_state(state, ref, step)  # the second process starts from what the first one stored


def test_two_processes_carry_the_state_through_the_file(torch_gpu, sets, tmp_path):
    _two_processes(sets, tmp_path, "A", "B", False)


def test_bf16_archives_over_an_fp32_master(torch_gpu, sets, tmp_path):
    """The replies are bf16; the state file holds the fp32 master the second step continues from."""
    _two_processes(sets, tmp_path, "A16", "B16", True)


def test_without_a_state_file_the_first_round_bootstraps(torch_gpu, sets, tmp_path):
    parts_dir, avg = sets["A"]
    state = tmp_path / "fresh.bin"
    out_dir = tmp_path / "replies"
    out_dir.mkdir()
    line = _round(parts_dir, out_dir, FLAGS + ["--server-state", str(state), "--eager"])  # --eager is accepted
    _line_ok(line, 0)
    _check_replies(out_dir, avg, False)  # plain FedAvg's bits
    _check_state(state, {mp: S.bootstrap(S.ADAM, avg[mp]) for mp in PARTS}, 0)


def test_a_state_of_another_size_ends_the_process(torch_gpu, sets, tmp_path):
    parts_dir, avg = sets["A"]
    state = tmp_path / "state.bin"
    z = np.zeros(5, F32)
    write_state(state, S.ADAM, {2: (z, z, z, 0)})
    base = pick_base()
    agg = subprocess.Popen([AGG, "-i", "-1", "-d", str(D), "-c", "1", "--rounds", "1", "--port-base", str(base)]
                           + FLAGS + ["--server-state", str(state)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True)
    owners = None
    out_dir = tmp_path / "replies"
    out_dir.mkdir()
    try:
        for line in agg.stderr:
            if "listening" in line:
                break
        owners = subprocess.Popen([REPLAY, "--dir", str(parts_dir), "--out", str(out_dir), "-d", str(D), "-c", "1",
                                   "--parts", "1,2,3", "--port-base", str(base)], stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True)
        out, err = agg.communicate(timeout=60)
        assert agg.returncode == 1, (agg.returncode, err[-2000:])
        assert "part 2" in err and " 5 " in err and str(avg[2].size) in err
    finally:
        for p in (agg, owners):
            if p is not None and p.poll() is None:
                p.kill()
                p.wait()
