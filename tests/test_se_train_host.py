"""CPU-side checks of the native squeeze-and-excitation training path (no GPU): the three C ABI additions are declared, listed
and exported and the ABI version did not move; fpc_se_bwd_scratch_floats follows its formula; both launching entries refuse null
and misaligned pointers and bad shapes before any launch; the switch is off by default; the front door refuses CPU tensors and an
SEResNetBottleneck on the CPU computes the same with the switch on; and the float64 reference the GPU tests are held to
(_se_train_refs.backward_ref, the kernels' formulas written out) IS torch.autograd through SEModule + add + ReLU in float64."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import _se_train_refs as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
ENTRIES = {      # name -> (result, arguments) as include/fpc.h declares them
    "fpc_se_gate_train": (_i, [_vp] * 9 + [_i] * 5 + [_vp]),
    "fpc_se_bwd_scratch_floats": (_sz, [_i] * 5),
    "fpc_se_bwd": (_i, [_vp] * 15 + [_i] * 5 + [_vp]),
}
NEW_KEYS = ("se_fwd_native", "se_bwd_native", "se_torch")


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def test_the_three_entries_are_declared_listed_and_exported(hiplib):
    from fastposecnn_amd import _native
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    cited = hdr[hdr.index("int fpc_se_gate_train") - 3500:hdr.index("int fpc_se_gate_train")]
    assert "F/lib/pose_regressor.py:608-613" in cited and "SEModule" in cited and "SEResNetBottleneck.forward" in cited
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
    assert re.search(r"#define\s+FPC_ABI_VERSION\s+11\b", hdr) and hiplib.fpc_abi_version() == 11


def test_bwd_scratch_floats_formula(hiplib):
    L = hiplib
    for B, H, W, C, Rd in R.SHAPES + [(8, 120, 160, 256, 16), (32, 15, 20, 2048, 16), (1, 1, 1, 8192, 1)]:
        slabs = L.fpc_se_pool_slabs(H, W, C)
        assert slabs >= 1
        assert L.fpc_se_bwd_scratch_floats(B, H, W, C, Rd) == B * (slabs * C + 2 * C + C // Rd), (B, H, W, C, Rd)
        assert L.fpc_se_bwd_scratch_floats(B, H, W, C, Rd) >= L.fpc_se_scratch_floats(B, H, W, C)
    for bad in [(0, 5, 7, 128, 16), (-1, 5, 7, 128, 16), (2, 5, 7, 96, 16), (2, 5, 7, 32, 16), (2, 5, 7, 0, 16), (2, 5, 7, 100, 4),
                (2, 5, 7, 8256, 16), (2, 5, 7, 128, 0), (2, 5, 7, 128, 3), (2, 0, 7, 128, 16), (2, 5, 0, 128, 16)]:
        assert L.fpc_se_bwd_scratch_floats(*bad) == 0, bad


def _host(n):
    """The address of a 16-byte-aligned host buffer of n floats (validation precedes any launch: it is never dereferenced)."""
    buf = ctypes.create_string_buffer(4 * n + 16)
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_refusals_come_before_any_launch(hiplib):
    L = hiplib
    B, H, W, C, Rd = 2, 5, 7, 128, 16
    keep = []

    def p(n):
        buf, a = _host(n)
        keep.append(buf)
        return a
    big, Cr = B * H * W * C, C // Rd
    gate_args = [p(big), p(Cr * C), p(Cr), p(C * Cr), p(C), p(B * C), p(B * C), p(B * Cr), p(L.fpc_se_scratch_floats(B, H, W, C))]
    bwd_args = [p(big), p(big), p(big), p(B * C), p(B * C), p(B * Cr), p(Cr * C), p(C * Cr), p(big), p(big), p(Cr * C), p(Cr), p(C * Cr),
                p(C), p(L.fpc_se_bwd_scratch_floats(B, H, W, C, Rd))]
    for fn, good, nullable in ((L.fpc_se_gate_train, gate_args, ()), (L.fpc_se_bwd, bwd_args, (9,))):
        for i in range(len(good)):
            args = list(good)
            args[i] = good[i] + 4
            assert fn(*args, B, H, W, C, Rd, None) == -1, ("misaligned", i)
            if i not in nullable:
                args[i] = None
                assert fn(*args, B, H, W, C, Rd, None) == -1, ("null", i)
        for C_bad in (96, 32, 0, 100, 8256):
            assert fn(*good, B, H, W, C_bad, 16, None) == -1, C_bad
        for R_bad in (0, -1, 3, 24, 256):
            assert fn(*good, B, H, W, C, R_bad, None) == -1, R_bad
        for B_bad in (0, -3, 65536):
            assert fn(*good, B_bad, H, W, C, Rd, None) == -1, B_bad
        assert fn(*good, B, 0, W, C, Rd, None) == -1 and fn(*good, B, H, -1, C, Rd, None) == -1
        assert fn(*good, B, 1 << 16, 1 << 16, C, Rd, None) == -1      # a shape se_shape_ok refuses: H W >= 2^31


def test_switch_is_off_when_the_variable_is_unset():
    env = {k: v for k, v in os.environ.items() if k != "FPC_TRAIN_NATIVE_SE"}
    code = ("from fastposecnn_amd.lib import train_conv\n"
            "assert train_conv.NATIVE_SE is False\n"
            "assert all(train_conv.counters[k] == 0 for k in %r)\n" % (NEW_KEYS,))
    subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, check=True, timeout=300)
    env["FPC_TRAIN_NATIVE_SE"] = "1"
    subprocess.run([sys.executable, "-c", code.replace("is False", "is True")], cwd=REPO, env=env, check=True, timeout=300)


@pytest.mark.parametrize("switch", [False, True])
def test_cpu_tensors_are_torch(monkeypatch, switch):
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_SE", switch)
    monkeypatch.setattr(train_conv, "ENABLED", True)
    torch.manual_seed(0)
    blk = bb.SEResNetBottleneck(256, 64, 16).train()
    assert sorted(k for k in blk.state_dict() if k.startswith("se_module")) == [
        "se_module.fc1.bias", "se_module.fc1.weight", "se_module.fc2.bias", "se_module.fc2.weight"]
    x = torch.randn((2, 256, 6, 5)).contiguous(memory_format=torch.channels_last)
    res = torch.randn_like(x)
    assert train_conv.se_gate_add_relu(x, blk.se_module, res, blk.relu) is None
    assert train_conv.se_gate_add_relu(x, blk.se_module, res) is None
    before = dict(train_conv.counters)
    blk.eval()          # (BatchNorm on its running statistics: the two calls below see the same module state)
    with torch.enable_grad():
        y = blk(x)
    out = blk.bn3(blk.conv3(blk.relu(blk.bn2(blk.conv2(blk.relu(blk.bn1(blk.conv1(x))))))))
    want = torch.relu(blk.se_module(out) + x)
    assert torch.equal(y, want)
    y.sum().backward()
    assert blk.se_module.fc1.weight.grad is not None and blk.se_module.fc1.weight.grad.shape == (16, 256, 1, 1)
    assert dict(train_conv.counters) == before


@pytest.mark.parametrize("case", R.SHAPES, ids=R.IDS)
def test_reference_is_autograd_in_float64(case):
    """The yardstick: the written-out formulas against torch.autograd.grad through backbone.SEModule + add + ReLU, float64."""
    from fastposecnn_amd.lib import backbone as bb
    B, H, W, C, Rd = case
    ops, ref = R.operands(case)
    assert ref["pre_out"].abs().min().item() >= 0.2 and ref["pre_hidden"].abs().min().item() >= 1e-3
    assert (ref["pre_hidden"][0].abs() >= 0.25 - 1e-5).all()
    se = bb.SEModule(C, Rd).double()
    with torch.no_grad():
        se.fc1.weight.copy_(ops["w1"].double().view(C // Rd, C, 1, 1)); se.fc1.bias.copy_(ops["b1"].double())
        se.fc2.weight.copy_(ops["w2"].double().view(C, C // Rd, 1, 1)); se.fc2.bias.copy_(ops["b2"].double())
    x = ops["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
    res = ops["res"].double().permute(0, 3, 1, 2).requires_grad_(True)
    y = torch.relu(se(x) + res)
    params = [se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias]
    grads = torch.autograd.grad(y, [x, res] + params, ops["gy"].double().permute(0, 3, 1, 2))
    got = {"y": y.detach().permute(0, 2, 3, 1), "dx": grads[0].permute(0, 2, 3, 1), "dres": grads[1].permute(0, 2, 3, 1),
           "dw1": grads[2].view(C // Rd, C), "db1": grads[3], "dw2": grads[4].view(C, C // Rd), "db2": grads[5]}
    for k, v in got.items():
        err = (v - ref[k]).abs().max().item()
        assert err <= 1e-12 * max(1.0, ref[k].abs().max().item()), (k, err)
    assert ref["dw1"].abs().max().item() > 0 and ref["dx"].abs().max().item() > 0
