"""End-to-end: --geomed-iters through the drop-in aggregator process over loopback TCP (GPU), and the flag
combinations it refuses while it parses its arguments (no GPU).

Five data owners send parts 1, 2 and 3 of the three modules of tests/test_f16_e2e.py; tests/replay_tool replays the
archive files and keeps every reply.  Owner slot 1 sends 1e30 in every parameter, the others 0.5 randn.  With
--geomed-iters 4 nobody is left out, but the round line's final weights give that owner less than a hundredth of its
fifth (the share s_t of an owner infinitely far away obeys s_{t+1} = s_0 r / (s_0 r + 1 - s_0), r = s_t / (1 - s_t):
0.2, 0.059, 0.015, 0.0039, 0.00098).  The final weights are bit-equal to rules 3-4 of fa.h "Geomed stage" applied
to the line's last-pass distances, every reply is bit-equal to the chain under those weights, and every stored
CRC-32 equals zlib's.
"""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import geomed_ref as G
from conftest import PKG_DIR, ROOT
from test_f16_e2e import _modules, pick_base
from test_server_opt_e2e import _reply_bits

AGG = os.path.join(PKG_DIR, "bin", "fa_aggregator")
REPLAY = os.path.join(ROOT, "tests", "tools", "bin", "fa_replay_owners")
D, T = 5, 4
F32 = np.float32
PARTS = [1, 2, 3]
FAR = 1  # the slot whose archives hold 1e30


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
                    p.copy_((torch.full(p.shape, 1e30) if k == FAR else torch.randn(p.shape).mul_(0.5)).to(p.dtype))
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
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "replay_tool")], check=True, capture_output=True)
    kind = "bf16" if bf16 else "f32"
    w = np.full(D, F32(1.0) / F32(D), F32)  # the aggregator's default weights
    parts_dir, out_dir = tmp_path / "parts", tmp_path / "replies"
    parts_dir.mkdir()
    out_dir.mkdir()
    xs = _write_parts(parts_dir, 1700, bf16)
    line, err = _round(parts_dir, out_dir, ["--geomed-iters", str(T)])
    assert line["geomed_iters"] == T and F32(line["geomed_nu"]) == F32(1e-6)
    owners = line["geomed_owners"]
    assert len(owners) == D and len(set(owners)) == D
    assert "NO OWNER LEFT" not in err
    for mp in PARTS:
        assert line["geomed_passes"][str(mp)] == T and line["geomed_excluded"][str(mp)] == []
        q = np.asarray([float(v) for v in line["geomed_sumsq"][str(mp)]], np.float64)
        alpha = np.asarray([F32(v) for v in line["geomed_weights"][str(mp)]], F32)
        rule, inc, _ = G.weights(w, q, np.ones(D, bool), 1e-6)
        assert inc.all()
        G.assert_bits(alpha, rule, "part %d: the final weights are rule 4 of the last pass's distances" % mp)
        assert alpha[FAR] < 0.01 * w[FAR], (mp, alpha)
        assert abs(float(alpha.astype(np.float64).sum()) - 1.0) < 1e-6
        want = G.round_out(G.aggregate_from_trace(O, xs[mp], kind, [alpha], inc), kind)
        assert np.isfinite(G.widen(want, kind)).all()
        files = sorted(glob.glob(str(out_dir / ("reply_mp%d_port*.pt" % mp))))
        assert len(files) == D
        for f in files:
            G.assert_bits(_reply_bits(f, bf16), want, os.path.basename(f))  # checks the CRC-32s too


@pytest.mark.gpu
def test_the_far_owner_is_down_weighted_in_every_bucket(torch_gpu, O, tmp_path):
    _one_round(tmp_path, O, False)


@pytest.mark.gpu
def test_bf16_archives(torch_gpu, O, tmp_path):
    _one_round(tmp_path, O, True)


# ------------------------------------------------------------------ the drop-in's flags (no GPU)

@pytest.mark.parametrize("args,says", [
    (["--geomed-iters", "4", "--clip-norm", "1"], "--clip-norm"),
    (["--geomed-iters", "4", "--krum-f", "1"], "--krum-f"),
    (["--geomed-iters", "4", "--mode", "literal"], "--mode literal"),
    (["--geomed-iters", "4", "--mode", "trimmed"], "--mode trimmed"),
    (["--geomed-iters", "4", "--mode", "median"], "--mode median"),
    (["--geomed-iters", "4", "--mode", "bulyan", "--bulyan-f", "0"], "--mode bulyan"),
    (["--geomed-iters", "4", "--layout", "rs"], "--layout rs"),
    (["--geomed-iters", "0"], "--geomed-iters 0"),
    (["--geomed-iters", "65"], "--geomed-iters 65"),
    (["--geomed-iters", "4", "--geomed-nu", "0"], "--geomed-nu 0"),
    (["--geomed-iters", "4", "--geomed-nu", "inf"], "--geomed-nu inf"),
    (["--geomed-nu", "1e-6"], "--geomed-iters"),  # nu without iters
])
def test_aggregator_flag_refusals_exit_2(args, says):
    """Refused while the arguments are parsed: usage on stderr, exit 2, before any device or socket is opened."""
    assert os.access(AGG, os.X_OK), "build the package first (make -C %s)" % PKG_DIR
    r = subprocess.run([AGG, "-i", "-1", "-c", "1", "-d", "5"] + args, capture_output=True, text=True, timeout=30)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert says in r.stderr and "usage: fa_aggregator" in r.stderr and "--geomed-iters T [--geomed-nu NU]" in r.stderr
    assert "listening" not in r.stderr and r.stdout == ""
