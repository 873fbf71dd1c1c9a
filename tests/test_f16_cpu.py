"""CPU tests of the fp16 bucket dtype (FA_F16): the rounding rule the GPU tests take as "expected", the
binding's constants, the launch plans (pure host arithmetic: fp16 takes exactly the bf16 plans, and the
bf16 <-> fp16 pairs are refused) and the archive reader on HalfStorage parameters."""
import io
import json
import os
import subprocess
import zipfile

import numpy as np
import pytest

from conftest import PKG_DIR

TOOL = os.path.join(PKG_DIR, "bin", "fa_archive_tool")
C3, C4_FC, C4_ALL, C5 = 42_737_546, 119_586_826, 139_611_210, 1 << 28
# every (n, clients) tests/test_plan.py plans, plus the fp16 bench row (C3's shape)
PLAN_SHAPES = [(64 << 20, 32), (C4_ALL, 64), (C4_FC, 64), (C5, 128), (16 << 20, 32), (8 << 20, 32), (12_557_962, 8),
               (1 << 20, 64), (C3, 32), (29_511_680, 32)]


def tool(*args, check=True):
    return subprocess.run([TOOL, *map(str, args)], capture_output=True, text=True, check=check)


def test_numpy_rounds_f32_to_f16_nearest_even():
    """What "expected" means in the fp16 tests: numpy's float32 -> float16 cast is round-to-nearest-even with
    overflow to inf and gradual underflow (the contract of FA_F16 outputs in fa.h)."""
    f = np.float32
    cases = [(f(65519.99), 0x7BFF), (f(65520), 0x7C00), (f(2.0 ** -24), 0x0001), (f(2.0 ** -25), 0x0000),
             (f(2.0 ** -25) * f(1.0001), 0x0001), (f(2.0 ** -14) * (f(1) - f(2.0 ** -11)), 0x0400),
             (f(1) + f(2.0 ** -11), 0x3C00), (f(1) + f(3) * f(2.0 ** -11), 0x3C02)]
    x = np.array([c[0] for c in cases], np.float32)
    with np.errstate(over="ignore"):
        got = x.astype(np.float16).view(np.uint16)
    assert got.tolist() == [c[1] for c in cases]
    # widening is exact, subnormals included
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    back = h.astype(np.float32).astype(np.float16)
    ok = ~np.isnan(h)
    assert np.array_equal(back.view(np.uint16)[ok], h.view(np.uint16)[ok])


def test_binding_constants(fa):
    assert (fa.F32, fa.BF16, fa.F16) == (0, 1, 2)
    assert fa.DTYPE_SIZE[fa.F16] == 2
    assert fa.lib().fa_version() == 7  # a new enum value is additive


@pytest.mark.parametrize("n,clients", PLAN_SHAPES)
def test_f16_takes_the_bf16_plans(fa, n, clients):
    for walk in (0, 2, 4, 5, 6):
        for cus in (256, 128):
            kw = dict(walk=walk, cus=cus)
            assert fa.plan_chain(fa.F16, fa.F16, n, clients, **kw) == fa.plan_chain(fa.BF16, fa.BF16, n, clients, **kw)
            assert fa.plan_chain(fa.F16, fa.F32, n, clients, **kw) == fa.plan_chain(fa.BF16, fa.F32, n, clients, **kw)
            assert fa.plan_chain(fa.F32, fa.F16, n, clients, **kw) == fa.plan_chain(fa.F32, fa.BF16, n, clients, **kw)


def test_f16_plans_named(fa):
    # the fp16 bench row: C3's two phases of the 512-thread form; one phase sized to a smaller bucket
    assert fa.plan_chain(fa.F16, fa.F16, C3, 32) == (fa.PLAN_PHASED, 2)
    assert fa.plan_chain(fa.F16, fa.F16, 29_511_680, 32) == (fa.PLAN_PHASED, 1)
    assert fa.piece_plan(C5, 128, fa.F16) == fa.piece_plan(C5, 128, fa.BF16) == (4, 1 << 26)
    for gpus in (1, 2, 8):
        assert fa.rs_plan(C4_ALL, gpus, 64, 0, fa.F16, fa.F16) == fa.rs_plan(C4_ALL, gpus, 64, 0, fa.BF16, fa.BF16)
        assert fa.rs_plan(C4_ALL, gpus, 64, 0, fa.F32, fa.F16) == fa.rs_plan(C4_ALL, gpus, 64, 0, fa.F32, fa.BF16)


@pytest.mark.parametrize("pair", ["bf16_f16", "f16_bf16"])
def test_mixed_16bit_pairs_are_refused(fa, pair):
    a, b = (fa.BF16, fa.F16) if pair == "bf16_f16" else (fa.F16, fa.BF16)
    with pytest.raises(fa.FaError) as e:
        fa.plan_chain(a, b, 1 << 20, 4)
    assert e.value.code == fa.ERR_ARG and "bf16" in str(e.value) and "f16" in str(e.value).replace("bf16", "")
    with pytest.raises(fa.FaError) as e:
        fa.rs_plan(1 << 20, 2, 4, 0, a, b)
    assert e.value.code == fa.ERR_ARG and "bf16" in str(e.value)


# ------------------------------------------------------------------ archives with HalfStorage parameters

def half_module(seed=11):
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 5, 3), nn.BatchNorm2d(5), nn.Flatten(), nn.Linear(20, 7)).half()


def flat_bits(m):
    import torch
    return torch.cat([p.detach().reshape(-1) for _, p in m.named_parameters()]).view(torch.int16).numpy().view(np.uint16)


def test_half_archive_is_reported_as_fp16(tmp_path):
    import torch
    m = half_module()
    src = tmp_path / "half.pt"
    torch.jit.save(torch.jit.script(m), str(src))
    d = json.loads(tool("dump", src).stdout)
    want = sum(p.numel() for p in m.parameters())
    assert d["param_dtype"] == "fp16" and d["param_elem_size"] == 2 and d["param_numel"] == want
    assert all(p["storage"] == "HalfStorage" for p in d["params"])
    tool("gather-bytes", src, tmp_path / "raw")
    raw = np.fromfile(tmp_path / "raw", np.uint16)
    assert raw.size == want and np.array_equal(raw, flat_bits(m))
    # the fp32-only entries say what they are
    r = tool("gather", src, tmp_path / "x", check=False)
    assert r.returncode != 0 and "fp32" in r.stderr


def test_patched_half_archive_loads_with_float16_parameters(tmp_path):
    import torch
    m = half_module()
    src = tmp_path / "half.pt"
    torch.jit.save(torch.jit.script(m), str(src))
    n = sum(p.numel() for p in m.parameters())
    vals = np.random.default_rng(2).standard_normal(n).astype(np.float16)
    vals.tofile(tmp_path / "v.f16")
    tool("patch-bytes", src, tmp_path / "v.f16", tmp_path / "out.pt")
    data = (tmp_path / "out.pt").read_bytes()
    assert zipfile.ZipFile(io.BytesIO(data)).testzip() is None
    got = torch.jit.load(io.BytesIO(data))
    assert all(p.dtype == torch.float16 for p in got.parameters())
    assert np.array_equal(flat_bits(got), vals.view(np.uint16))
    for (na, a), (nb, b) in zip(got.named_buffers(), m.named_buffers()):
        assert na == nb and torch.equal(a, b)


def test_archive_mixing_half_and_bfloat16_is_refused(tmp_path):
    import torch
    import torch.nn as nn
    m = nn.Sequential(nn.Linear(4, 3).half(), nn.Linear(3, 2).to(torch.bfloat16))
    src = tmp_path / "mixed.pt"
    torch.jit.save(torch.jit.script(m), str(src))
    d = json.loads(tool("dump", src).stdout)
    assert d["param_dtype"] == "none" and d["param_elem_size"] == 0
    assert {p["storage"] for p in d["params"]} == {"HalfStorage", "BFloat16Storage"}
    r = tool("gather-bytes", src, tmp_path / "raw", check=False)
    assert r.returncode != 0 and "fp16" in r.stderr
    # a whole-bf16 archive stays bf16: the two 2-byte types are told apart by storage, not by size
    mb = nn.Sequential(nn.Linear(4, 3)).to(torch.bfloat16)
    torch.jit.save(torch.jit.script(mb), str(tmp_path / "bf.pt"))
    assert json.loads(tool("dump", tmp_path / "bf.pt").stdout)["param_dtype"] == "bf16"


def test_compute_states_accept_float16():
    """ClientStates packs torch.float16 modules and hands fa.F16 to the sync (checked with a stand-in sync)."""
    import torch
    import torch.nn as nn
    from conftest import load_pkg
    load_pkg()
    from mhfsl_amd.compute import ClientStates
    mods = {c: nn.Linear(6, 3).half() for c in (4, 9)}
    seen = {}
    st = ClientStates(mods, sync_fn=lambda slots, w, n: seen.update(n=n, dt=slots[0].dtype))
    st.aggregate()
    assert st.dtype == torch.float16 and seen == {"n": 21, "dt": torch.float16}
    assert st.stride * 2 % 16 == 0
