"""CPU-side checks of the native VGG training path (no GPU): the references themselves on hand-computed cases, the four C ABI
additions declared, exported and listed with the signatures _native.py gives them, the ABI version where it was, the slice count and
the workspace size agreeing with each other and 0 for refused shapes, the switch off by default, and with it off — or on CPU tensors
with it on — conv2d(), maxpool2x2() and VGGEncoder.forward being torch's own, bit for bit."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _vgg_train_refs as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
ENTRIES = {      # name -> (result, arguments) as include/fpc.h declares them
    "fpc_conv3x3_c3_wgrad_workspace_bytes": (_sz, [_i, _i, _i]),
    "fpc_conv3x3_c3_wgrad_slices": (_i, [_i, _i, _i]),
    "fpc_conv3x3_c3_wgrad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "fpc_maxpool2x2_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
}
NEW_KEYS = ("c3_fwd_native", "c3_wgrad_native", "pool2_fwd_native", "pool2_bwd_native")


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def test_wgrad_reference_on_a_1x1_image():
    """One pixel: only the centre tap sees it — dw[co][ci][1][1] = dy[co] img[ci], every other tap 0, db = dy."""
    img = torch.tensor([2.0, -3.0, 5.0]).view(1, 3, 1, 1)
    dy = torch.arange(64, dtype=torch.float32).view(1, 64, 1, 1) - 7.0
    dw, db = R.c3_wgrad_ref(img, dy)
    want = torch.zeros((64, 3, 3, 3), dtype=torch.float64)
    want[:, :, 1, 1] = dy.view(64, 1).double() * img.view(1, 3).double()
    assert torch.equal(dw, want) and torch.equal(db, dy.view(64).double())


def test_wgrad_reference_tap_orientation():
    """dy one-hot at the top-left pixel of a 2 x 2 image of distinct values: tap (kh, kw) reads img[kh - 1][kw - 1] — no flip —,
    taps that fall outside the image are 0."""
    img = torch.arange(1.0, 13.0).view(1, 3, 2, 2)
    dy = torch.zeros((1, 64, 2, 2))
    dy[0, 5, 0, 0] = 1.0
    dw, db = R.c3_wgrad_ref(img, dy)
    want = torch.zeros((64, 3, 3, 3), dtype=torch.float64)
    want[5, :, 1:, 1:] = img[0].double()
    assert torch.equal(dw, want) and db[5] == 1.0 and db.sum() == 1.0


def test_pool_reference_on_four_equal_values():
    """A window of four equal values: the gradient goes to element (0, 0) alone (torch's first maximum, a strict >)."""
    x = torch.full((1, 1, 2, 2), 0.5)
    y, dx = R.pool2_ref(x, torch.full((1, 1, 1, 1), 3.0))
    assert torch.equal(y, torch.full((1, 1, 1, 1), 0.5, dtype=torch.float64))
    assert torch.equal(dx, torch.tensor([[3.0, 0.0], [0.0, 0.0]], dtype=torch.float64).view(1, 1, 2, 2))
    # ... and to the planted maximum otherwise, at each of the four positions
    for kind, xs in R.pool_inputs(1, 2, 2, 4, 3).items():
        if kind.startswith("max at"):
            k = int(kind[-1])
            _, dx = R.pool2_ref(xs, torch.ones((1, 4, 1, 1)))
            want = torch.zeros((1, 4, 2, 2), dtype=torch.float64)
            want[:, :, k // 2, k % 2] = 1.0
            assert torch.equal(dx, want), kind
    eq = R.pool_inputs(2, 4, 6, 4, 4)["equal"]
    _, dx = R.pool2_ref(eq, torch.ones((2, 4, 2, 3)))
    assert torch.equal(dx[:, :, ::2, ::2], torch.ones((2, 4, 2, 3), dtype=torch.float64)) and dx.sum() == 2 * 4 * 2 * 3


def test_the_four_entries_are_declared_listed_and_exported(hiplib):
    from fastposecnn_amd import _native
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    at = hdr.index("size_t fpc_conv3x3_c3_wgrad_workspace_bytes")
    assert "F/lib/pose_regressor.py:608" in hdr[at - 3000:at] and "FPC_TRAIN_NATIVE_VGG" in hdr[at - 3000:at]
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
    for shape in [(0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 64, 64), (2 ** 20, 64, 64), (1, 2 ** 14, 2 ** 14)]:      # the last two: B H W = 2^28
        assert L.fpc_conv3x3_c3_wgrad_slices(*shape) == 0 and L.fpc_conv3x3_c3_wgrad_workspace_bytes(*shape) == 0, shape
    seen = set()
    for shape in [(1, 1, 1), (1, 2, 3), (2, 5, 7), (1, 33, 65), (3, 32, 96), (2, 37, 70), (8, 480, 640), (32, 480, 640), (873, 480, 640)]:
        n, nbytes = L.fpc_conv3x3_c3_wgrad_slices(*shape), L.fpc_conv3x3_c3_wgrad_workspace_bytes(*shape)
        B, H, W = shape
        units = B * H * ((W + 63) // 64)
        assert 1 <= n <= units, (shape, n)
        assert nbytes == n * 64 * 48 * 4, (shape, n, nbytes)
        assert (n, nbytes) == (L.fpc_conv3x3_c3_wgrad_slices(*shape), L.fpc_conv3x3_c3_wgrad_workspace_bytes(*shape))      # of the shape alone
        seen.add(n)
    assert 1 in seen and len(seen) >= 4


def test_switch_is_off_when_the_variable_is_unset():
    env = {k: v for k, v in os.environ.items() if k != "FPC_TRAIN_NATIVE_VGG"}
    code = ("from fastposecnn_amd.lib import train_conv\n"
            "assert train_conv.NATIVE_VGG is False\n"
            "assert all(train_conv.counters[k] == 0 for k in %r)\n" % (NEW_KEYS,))
    subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, check=True, timeout=300)
    env["FPC_TRAIN_NATIVE_VGG"] = "1"
    subprocess.run([sys.executable, "-c", code.replace("is False", "is True")], cwd=REPO, env=env, check=True, timeout=300)


@pytest.mark.parametrize("switch", [False, True])
def test_cpu_tensors_and_the_switch_off_are_torch(monkeypatch, switch):
    """The gates refuse: maxpool2x2 returns None, conv2d on a (64, 3, 3, 3) weight reaches F.conv2d, no counter moves."""
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_VGG", switch)
    monkeypatch.setattr(train_conv, "ENABLED", True)
    g = torch.Generator().manual_seed(0)
    x = torch.randn((2, 3, 16, 24), generator=g)
    before = dict(train_conv.counters)
    for bias in (True, False):
        conv = bb.Conv2d(3, 64, 3, padding=1, bias=bias).train()
        assert tuple(conv.weight.shape) == (64, 3, 3, 3)
        assert not train_conv._vgg_c3_ok(x, conv.weight, conv.bias, 1, 1)
        y = conv(x)
        assert torch.equal(y, F.conv2d(x, conv.weight, conv.bias, 1, 1))
        assert torch.equal(train_conv.conv2d(x, conv.weight, conv.bias, 1, 1), F.conv2d(x, conv.weight, conv.bias, 1, 1))
    assert y.requires_grad and train_conv.maxpool2x2(y) is None
    assert train_conv.maxpool2x2(y.contiguous(memory_format=torch.channels_last)) is None
    y.sum().backward()
    assert conv.weight.grad is not None
    assert dict(train_conv.counters) == before


@pytest.mark.parametrize("name", ["vgg11", "vgg11_bn"])
def test_vgg_encoder_on_the_cpu_is_unchanged_with_the_switch_forced_on(monkeypatch, name):
    """VGGEncoder.forward asks maxpool2x2 for its pools; off the GPU everything is refused, so the six feature levels and the
    gradients are those of the plain module chain, bit for bit."""
    from fastposecnn_amd.lib import backbone as bb, train_conv
    torch.manual_seed(3)
    enc = bb.VGGEncoder(name).train()
    x = torch.randn((2, 3, 32, 64), generator=torch.Generator().manual_seed(4))
    sd = {k: v.clone() for k, v in enc.state_dict().items()}

    def chain(inp):      # the module chain as nn.Sequential would run it, split at the pools
        feats = []
        for m in enc.features:
            if isinstance(m, torch.nn.MaxPool2d):
                feats.append(inp)
            inp = m(inp)
        return feats + [inp]

    monkeypatch.setattr(train_conv, "NATIVE_VGG", False)
    want = chain(x)
    gwant = torch.autograd.grad(sum(f.square().mean() for f in want), enc.features[0].weight)[0]
    enc.load_state_dict(sd)      # (the BatchNorms' running statistics moved)
    monkeypatch.setattr(train_conv, "NATIVE_VGG", True)
    monkeypatch.setattr(train_conv, "ENABLED", True)
    before = dict(train_conv.counters)
    got = enc(x)
    ggot = torch.autograd.grad(sum(f.square().mean() for f in got), enc.features[0].weight)[0]
    assert len(got) == len(want) == 6
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(ggot, gwant)
    assert dict(train_conv.counters) == before
