"""CPU: TorchArchive::mx8_view over bytes from the wire, under AddressSanitizer and UBSan.

tests/mx8_tool/mx8_archive_check.cpp is a stand-alone program (its own main, built with -fsanitize=address,undefined,
run as its own process): it parses a good MX8 receipt, every truncation of it, and archives that are almost one -- a
scale buffer one short and one long, a float parameter, two parameters, the buffer and the parameter swapped -- and
reads every byte of every view it is handed.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "tests", "tools", "bin")
N = 1000


@pytest.fixture(scope="module", autouse=True)
def built():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "mx8_tool"), os.path.join(BIN, "mx8_archive_check_asan")],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.fail("sanitizer build failed:\n" + r.stderr[-3000:])


def save(path, params, buffers):
    """A scripted module with the given parameters and buffers (name -> tensor), as the owners save theirs."""
    import torch
    import torch.nn as nn

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            for k, v in params.items():
                self.register_parameter(k, nn.Parameter(v, requires_grad=False))
            for k, v in buffers.items():
                self.register_buffer(k, v)

        def forward(self, x):
            return x

    torch.jit.save(torch.jit.script(M()), str(path))


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    import torch
    d = tmp_path_factory.mktemp("mx8_archives")
    rng = np.random.default_rng(8)
    q = torch.from_numpy(rng.integers(-128, 128, N).astype(np.int8))
    e = torch.from_numpy(rng.integers(0, 256, (N + 31) // 32).astype(np.uint8))
    save(d / "good.pt", {"q": q}, {"e": e})
    bad = {
        "scale one short": ({"q": q}, {"e": e[:-1].clone()}),
        "scale one long": ({"q": q}, {"e": torch.cat([e, e[:1]])}),
        "float parameter": ({"q": q.float()}, {"e": e}),
        "two parameters": ({"q": q, "r": q.clone()}, {"e": e}),
        "two buffers": ({"q": q}, {"e": e, "f": e.clone()}),
        "no buffer": ({"q": q}, {}),
        "swapped": ({"q": e.clone()}, {"e": q.clone()}),
        "strided codes": ({"q": torch.stack([q, q], 1)[:, 0]}, {"e": e}),
    }
    for name, (p, b) in bad.items():
        save(d / (name.replace(" ", "_") + ".pt"), p, b)
    want_sum = int(q.numpy().view(np.uint8).astype(np.int64).sum() + e.numpy().astype(np.int64).sum())
    return d, [str(d / (name.replace(" ", "_") + ".pt")) for name in bad], want_sum


def test_mx8_view_under_asan_ubsan(archives):
    d, bad, want_sum = archives
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(BIN, "mx8_archive_check_asan"), str(d / "good.pt")] + bad, capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["good"] == 1 and res["n"] == N and res["sum"] == want_sum  # the views are the tensors' bytes
    assert res["truncations"] == os.path.getsize(str(d / "good.pt")) and res["truncations_accepted"] == 0
    assert res["bad"] == len(bad) and res["bad_accepted"] == 0, r.stderr[-2000:]
