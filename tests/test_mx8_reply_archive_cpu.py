"""CPU: TorchArchive::with_mx8_into -- an MX8 reply patched into the owner's own receipt archive -- under AddressSanitizer
and UBSan.

tests/mx8_reply_tool/mx8_reply_patch_check.cpp is a stand-alone program (its own main, built with
-fsanitize=address,undefined, run as its own process): it patches new codes and scales into a good MX8 receipt, checks
every record's stored CRC-32 against zlib's, and feeds the patcher another n, null pointers, every truncation of the
receipt and archives that are almost one.  Here the patched archive is read once more with zipfile and torch.jit.load.
"""
import io
import json
import os
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_mx8_archive_cpu import save

BIN = os.path.join(ROOT, "tests", "tools", "bin")
N = 1000


@pytest.fixture(scope="module", autouse=True)
def built():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "mx8_reply_tool"),
                        os.path.join(BIN, "mx8_reply_patch_check_asan")], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.fail("sanitizer build failed:\n" + r.stderr[-3000:])


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    import torch
    d = tmp_path_factory.mktemp("mx8_reply_archives")
    rng = np.random.default_rng(9)
    q = torch.from_numpy(rng.integers(-128, 128, N).astype(np.int8))
    e = torch.from_numpy(rng.integers(0, 256, (N + 31) // 32).astype(np.uint8))
    save(d / "good.pt", {"q": q}, {"e": e})
    bad = {
        "one code more": ({"q": torch.cat([q, q[:1]])}, {"e": e}),
        "one block more": ({"q": torch.cat([q, q[:32]])}, {"e": torch.cat([e, e[:1]])}),
        "scale one short": ({"q": q}, {"e": e[:-1].clone()}),
        "float parameter": ({"q": q.float()}, {"e": e}),
        "two parameters": ({"q": q, "r": q.clone()}, {"e": e}),
        "no buffer": ({"q": q}, {}),
        "swapped": ({"q": e.clone()}, {"e": q.clone()}),
        "strided codes": ({"q": torch.stack([q, q], 1)[:, 0]}, {"e": e}),
        "full receipt": ({"w": torch.randn(N)}, {}),
    }
    for name, (p, b) in bad.items():
        save(d / (name.replace(" ", "_") + ".pt"), p, b)
    new_q = rng.integers(-127, 128, N).astype(np.int8)
    new_e = rng.integers(0, 256, (N + 31) // 32).astype(np.uint8)
    new_q.tofile(str(d / "q.bin"))
    new_e.tofile(str(d / "e.bin"))
    return d, [str(d / (name.replace(" ", "_") + ".pt")) for name in bad], new_q, new_e


def test_with_mx8_into_under_asan_ubsan(archives):
    import torch
    d, bad, new_q, new_e = archives
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(BIN, "mx8_reply_patch_check_asan"), str(d / "good.pt"), str(d / "q.bin"),
                        str(d / "e.bin"), str(d / "out.pt")] + bad, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["good"] == 1 and res["n"] == N and res["same"] == 1
    assert res["records"] > 2 and res["crc_ok"] == res["records"]
    assert res["refused_wrong"] == 6 and res["dirty"] == 0
    assert res["truncations"] == os.path.getsize(str(d / "good.pt")) and res["truncations_patched"] == 0
    assert res["bad"] == len(bad) and res["bad_patched"] == 0, r.stderr[-2000:]
    # the patched archive, read by others: zlib's CRC-32 over every record, and the owner's loader
    data = open(str(d / "out.pt"), "rb").read()
    assert len(data) == os.path.getsize(str(d / "good.pt"))
    zf = zipfile.ZipFile(io.BytesIO(data))
    for info in zf.infolist():
        assert zlib.crc32(zf.read(info.filename)) & 0xFFFFFFFF == info.CRC, info.filename
    m = torch.jit.load(io.BytesIO(data))
    assert np.array_equal(m.q.detach().numpy(), new_q) and np.array_equal(m.e.numpy(), new_e)
