"""CPU-side checks of the native stem / max-pool training path (no GPU): the six C ABI additions are declared, exported and
listed with the signatures _native.py gives them, the ABI version did not move, the slice count and the workspace size agree
with each other and are 0 for refused shapes, the gather rule the max-pool's backward implements IS torch's (bit for bit on
tie-heavy inputs), the switch is off by default, and with it off — or on CPU tensors — conv2d() and backbone.MaxPool2d are torch."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stem_refs as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
ENTRIES = {      # name -> (result, arguments) as include/fpc.h declares them
    "fpc_image_nhwc4": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "fpc_stem_wgrad_workspace_bytes": (_sz, [_i, _i, _i]),
    "fpc_stem_wgrad_slices": (_i, [_i, _i, _i]),
    "fpc_stem_wgrad": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "fpc_maxpool3x3s2_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "fpc_maxpool3x3s2_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
}
NEW_KEYS = ("stem_fwd_native", "stem_wgrad_native", "pool_fwd_native", "pool_bwd_native")


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def test_the_six_entries_are_declared_listed_and_exported(hiplib):
    from fastposecnn_amd import _native
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    assert "F/lib/pose_regressor.py:608" in hdr[hdr.index("fpc_image_nhwc4") - 3000:hdr.index("fpc_image_nhwc4")]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, (res, args) in ENTRIES.items():
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/fpc.h"
        assert len(m.group(2).split(",")) == len(args), (name, m.group(2))
        assert m.group(1) == ("size_t" if res is _sz else "int")
        assert name in _native.EXPORTED
        assert _native._SIGNATURES[name] == (res, args), name
        assert hasattr(raw, name), f"{name} is not exported"


def test_abi_version_is_still_11(hiplib):
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    assert re.search(r"#define\s+FPC_ABI_VERSION\s+11\b", hdr)
    assert hiplib.fpc_abi_version() == 11


def test_slices_and_workspace_bytes(hiplib):
    L = hiplib
    for shape in [(0, 8, 8), (1, 6, 8), (1, 8, 6), (1, 9, 8), (1, 8, 9), (-1, 64, 64), (1, 0, 0), (2 ** 20, 64, 64)]:
        assert L.fpc_stem_wgrad_slices(*shape) == 0 and L.fpc_stem_wgrad_workspace_bytes(*shape) == 0, shape
    seen = set()
    for shape in [(1, 8, 8), (2, 38, 70), (3, 64, 160), (2, 96, 256), (8, 480, 640), (32, 480, 640), (1, 8, 2048)]:
        n, nbytes = L.fpc_stem_wgrad_slices(*shape), L.fpc_stem_wgrad_workspace_bytes(*shape)
        B, Hi, Wi = shape
        units = B * (Hi // 2) * ((Wi // 2 + 63) // 64)
        assert 1 <= n <= units, (shape, n)
        assert nbytes >= n * 64 * 224 * 4 and nbytes % 256 == 0, (shape, n, nbytes)
        assert (n, nbytes) == (L.fpc_stem_wgrad_slices(*shape), L.fpc_stem_wgrad_workspace_bytes(*shape))      # of the shape alone
        seen.add(n)
    assert 1 in seen and len(seen) >= 4


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 4, 6, 10), (2, 3, 8, 8), (1, 2, 1, 1), (1, 2, 2, 5), (1, 3, 19, 12)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gather_rule_is_torchs_rule(shape, dtype):
    """relu(randn) (half exact zeros) with a constant plane; integer and random dy; odd and even sizes.  The numpy restatement of
    the rule equals CPU autograd bit for bit (one to four addends in the same order), and f32 equals float64 on integer dy."""
    x = R.tie_heavy(shape, 11, dtype)
    assert x.numel() < 100 or (x == 0).double().mean().item() >= 0.25
    g = torch.Generator().manual_seed(12)
    Ho, Wo = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
    for dy in (torch.randint(-3, 4, shape[:2] + (Ho, Wo), generator=g).to(dtype), torch.randn(shape[:2] + (Ho, Wo), generator=g).to(dtype)):
        _, want = R.maxpool_ref(x, dy)
        got = R.maxpool_bwd_gather(x.numpy(), dy.numpy())
        assert not np.isnan(got).any()
        assert np.array_equal(got, want.numpy())
        assert np.array_equal(R.maxpool_bwd_gather(x.contiguous(memory_format=torch.channels_last).numpy(), dy.numpy()), want.numpy())
    # a constant plane's gradient goes to the first in-bounds element of each window
    ones = torch.ones((1, 1, shape[2], shape[3]), dtype=dtype)
    dy1 = torch.ones((1, 1, Ho, Wo), dtype=dtype)
    got = R.maxpool_bwd_gather(ones.numpy(), dy1.numpy())[0, 0]
    want = np.zeros((shape[2], shape[3]))
    for oy in range(Ho):
        for ox in range(Wo):
            want[max(2 * oy - 1, 0), max(2 * ox - 1, 0)] += 1
    assert np.array_equal(got, want) and np.array_equal(R.maxpool_ref(ones, dy1)[1][0, 0].numpy(), want)


def test_f32_and_f64_autograd_agree_on_integer_dy():
    x = R.tie_heavy((2, 6, 7, 9), 5)
    dy = torch.randint(-3, 4, (2, 6, 4, 5), generator=torch.Generator().manual_seed(6)).float()
    assert torch.equal(R.maxpool_ref(x, dy)[1].double(), R.maxpool_ref(x.double(), dy.double())[1])


def test_switch_is_off_when_the_variable_is_unset():
    env = {k: v for k, v in os.environ.items() if k != "FPC_TRAIN_NATIVE_STEM"}
    code = ("from fastposecnn_amd.lib import train_conv\n"
            "assert train_conv.NATIVE_STEM is False\n"
            "assert all(train_conv.counters[k] == 0 for k in %r)\n" % (NEW_KEYS,))
    subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, check=True, timeout=300)
    env["FPC_TRAIN_NATIVE_STEM"] = "1"
    subprocess.run([sys.executable, "-c", code.replace("is False", "is True")], cwd=REPO, env=env, check=True, timeout=300)


@pytest.mark.parametrize("switch", [False, True])
def test_cpu_tensors_and_the_switch_off_are_torch(monkeypatch, switch):
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_STEM", switch)
    monkeypatch.setattr(train_conv, "ENABLED", True)
    g = torch.Generator().manual_seed(0)
    x = torch.randn((2, 3, 16, 24), generator=g)
    before = dict(train_conv.counters)
    conv = bb.Conv2d(3, 64, 7, 2, 3, bias=False).train()
    y = conv(x)
    assert torch.equal(y, F.conv2d(x, conv.weight, None, 2, 3))
    assert torch.equal(train_conv.conv2d(x, conv.weight, None, 2, 3), F.conv2d(x, conv.weight, None, 2, 3))
    pool = bb.MaxPool2d(3, 2, 1)
    assert isinstance(pool, torch.nn.MaxPool2d) and not list(pool.state_dict())
    want, gwant = R.maxpool_ref(y.detach(), torch.ones_like(F.max_pool2d(y.detach(), 3, 2, 1)))
    z = pool(y)
    assert torch.equal(z, want)
    z.sum().backward()
    assert conv.weight.grad is not None
    assert train_conv.maxpool3x3s2(y) is None
    assert dict(train_conv.counters) == before


def test_the_encoders_max_pool_is_the_subclass():
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.ResNetEncoder("resnet18")
    assert type(enc.maxpool) is bb.MaxPool2d
    assert (enc.maxpool.kernel_size, enc.maxpool.stride, enc.maxpool.padding) == (3, 2, 1)
    assert not any(k.startswith("maxpool") for k in enc.state_dict())
