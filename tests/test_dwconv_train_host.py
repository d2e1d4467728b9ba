"""CPU-side checks of the native depthwise / ReLU6 training path (no GPU): the five C ABI additions are declared, listed and
exported and the ABI version did not move; fpc_dwconv3x3_wgrad_workspace_bytes follows include/fpc.h's slice formula; every new
entry refuses null and misaligned pointers, bad shapes, a bad activation code and a bad workspace before any launch; the switch is
off by default; CPU tensors stay torch's with the switch on; and the float64 references the GPU tests are held to
(_dwconv_train_refs: the kernels' formulas written out) ARE torch.autograd through F.conv2d(groups = C) in float64."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import _dwconv_train_refs as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_vp, _i, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
ENTRIES = {      # name -> (result, arguments) as include/fpc.h declares them
    "fpc_dwconv3x3_dgrad": (_i, [_vp] * 3 + [_i] * 5 + [_vp]),
    "fpc_dwconv3x3_wgrad_workspace_bytes": (_sz, [_i] * 4),
    "fpc_dwconv3x3_wgrad": (_i, [_vp] * 3 + [_i] * 5 + [_vp, _sz, _vp]),
    "fpc_batchnorm_act_fwd": (_i, [_vp] * 9 + [_i, _i, _f, _f, _i, _vp]),
    "fpc_batchnorm_act_bwd": (_i, [_vp] * 10 + [_i, _i, _i, _vp]),
}
NEW_KEYS = ("dw_fwd_native", "dw_dgrad_native", "dw_wgrad_native", "bn_relu6_native")
EINVAL, EWORKSPACE = -1, -2
WALK_LIMIT = 2 ** 32 - 4096 * 256 - 8


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def test_the_five_entries_are_declared_listed_and_exported(hiplib):
    from fastposecnn_amd import _native
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    cited = hdr[hdr.index("int fpc_dwconv3x3_dgrad") - 3500:hdr.index("int fpc_dwconv3x3_dgrad")]
    assert "F/lib/pose_regressor.py:608-613" in cited and "torch.nn.Conv2d(groups = C)" in cited and "nn.ReLU6" in cited
    top = hdr[:hdr.index("#define FPC_ABI_VERSION")]
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
        assert name.replace("_workspace_bytes", "") in top, f"{name} is missing from the additions list"
    assert re.search(r"#define\s+FPC_ABI_VERSION\s+11\b", hdr) and hiplib.fpc_abi_version() == 11


def test_workspace_formula(hiplib):
    L = hiplib
    shapes = [(B, *R.out_hw(Hi, Wi, s), C) for B, Hi, Wi, C, s in R.CASES_ALL]
    shapes += [(8, 240, 320, 32), (8, 120, 160, 96), (8, 15, 20, 960), (8, 30, 40, 192), (1, 1, 1, 4), (1, 1, 300, 4), (64, 1, 1, 2048)]
    for B, Ho, Wo, C in shapes:
        n = R.wgrad_slices(B, Ho, Wo, C)
        assert 1 <= n <= max(1, min(1024, B * Ho))
        assert L.fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C) == n * C * 36, (B, Ho, Wo, C)
    # where the seams of the GPU file's two extra shapes fall
    (B, Hi, Wi, C, s), small = R.WGRAD_EXTRA[0], R.WGRAD_EXTRA[1]
    Ho, Wo = R.out_hw(Hi, Wi, s)
    assert (B * Ho, R.wgrad_slices(B, Ho, Wo, C)) == (22, 3) and [i * 22 // 3 for i in range(4)] == [0, 7, 14, 22]
    Ho, Wo = R.out_hw(small[1], small[2], small[4])
    assert R.wgrad_slices(small[0], Ho, Wo, small[3]) == 1 and small[0] * Ho * ((Wo + 7) // 8) < 32
    assert R.wgrad_slices(2, 17, 33, 16) == 5 and 34 % 5 != 0          # a forward case whose rows the slices do not divide either
    for bad in [(0, 5, 7, 32), (-1, 5, 7, 32), (2, 0, 7, 32), (2, 5, 0, 32), (2, 5, 7, 0), (2, 5, 7, 6), (2, 5, 7, 2), (2, 5, 7, -4),
                (1 << 15, 1 << 10, 1 << 10, 4)]:
        assert L.fpc_dwconv3x3_wgrad_workspace_bytes(*bad) == 0, bad


def _host(n):
    """The address of a 256-byte-aligned host buffer of n floats (validation precedes any launch: it is never dereferenced)."""
    buf = ctypes.create_string_buffer(4 * n + 256)
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 256


def test_depthwise_refusals_come_before_any_launch(hiplib):
    L = hiplib
    B, H, W, C = 2, 5, 7, 32
    keep = []

    def p(n):
        buf, a = _host(n)
        keep.append(buf)
        return a
    big = B * H * W * C
    need = L.fpc_dwconv3x3_wgrad_workspace_bytes(B, H, W, C)
    assert need > 0
    dgrad = lambda ptrs, B_=B, H_=H, W_=W, C_=C, s=1: L.fpc_dwconv3x3_dgrad(*ptrs, B_, H_, W_, C_, s, None)
    wgrad = lambda ptrs, B_=B, H_=H, W_=W, C_=C, s=1, ws=None, nb=need: L.fpc_dwconv3x3_wgrad(*ptrs, B_, H_, W_, C_, s, ws or wsp, nb, None)
    wsp = p(need // 4)
    for fn, good in ((dgrad, [p(big), p(9 * C), p(big)]), (wgrad, [p(big), p(big), p(9 * C)])):
        for i in range(3):
            args = list(good)
            args[i] = good[i] + 4
            assert fn(args) == EINVAL, ("misaligned", i)
            args[i] = None
            assert fn(args) == EINVAL, ("null", i)
        for B_bad in (0, -2):
            assert fn(good, B_=B_bad) == EINVAL
        for C_bad in (0, 2, 6, -4, 30):
            assert fn(good, C_=C_bad) == EINVAL, C_bad
        for s_bad in (0, 3, -1, 4):
            assert fn(good, s=s_bad) == EINVAL, s_bad
        assert fn(good, H_=0) == EINVAL and fn(good, W_=0) == EINVAL and fn(good, H_=-3) == EINVAL
        # an item count past the 32-bit walk limit: B Hi Wi C / 4 quads
        assert (1 << 11) * (1 << 11) * (1 << 10) * 1 >= WALK_LIMIT
        assert fn(good, B_=1 << 10, H_=1 << 11, W_=1 << 11, C_=4) == EINVAL
    wgood = [p(big), p(big), p(9 * C)]
    assert L.fpc_dwconv3x3_wgrad(*wgood, B, H, W, C, 1, None, need, None) == EINVAL             # a null workspace
    assert wgrad(wgood, ws=wsp + 16) == EWORKSPACE                                               # not 256-byte aligned
    assert wgrad(wgood, nb=need - 1) == EWORKSPACE and wgrad(wgood, nb=0) == EWORKSPACE          # too small


def test_batchnorm_act_refusals_come_before_any_launch(hiplib):
    L = hiplib
    P, C = 40, 64
    keep = []

    def p(n):
        buf, a = _host(n)
        keep.append(buf)
        return a
    x, res, y, dy, dx, dres = (p(P * C) for _ in range(6))
    gamma, beta, rm, rv, dg, db, stats = (p(2 * C) for _ in range(7))
    part = p(L.fpc_batchnorm_scratch_floats(P, C))

    def fwd(act, res_=None, x_=x, P_=P, C_=C, gamma_=gamma):
        return L.fpc_batchnorm_act_fwd(x_, res_, gamma_, beta, rm, rv, y, stats, part, P_, C_, 1e-5, 0.1, act, None)

    def bwd(act, dres_=None, x_=x, P_=P, C_=C, gamma_=gamma, y_=y):
        return L.fpc_batchnorm_act_bwd(x_, y_, dy, gamma_, stats, dx, dres_, dg, db, part, P_, C_, act, None)

    for call in (fwd, bwd):
        for act in (3, -1, 7):
            assert call(act) == EINVAL, act
        for act in (0, 1, 2):
            assert call(act, C_=6) == EINVAL and call(act, P_=1) == EINVAL
            assert call(act, gamma_=None) == EINVAL and call(act, x_=x + 4) == EINVAL and call(act, x_=None) == EINVAL
    assert fwd(2, res_=res) == EINVAL and fwd(0, res_=res) == EINVAL      # a residual goes with ReLU alone
    assert bwd(2, dres_=dres) == EINVAL and bwd(0, dres_=dres) == EINVAL
    assert bwd(2, y_=None) == EINVAL and bwd(1, y_=None) == EINVAL        # the mask needs the saved output
    # the old entries keep refusing what they refused
    assert L.fpc_batchnorm_fwd(x, res, gamma, beta, rm, rv, y, stats, part, P, C, 1e-5, 0.1, 0, None) == EINVAL
    assert L.fpc_batchnorm_fwd(x + 4, None, gamma, beta, rm, rv, y, stats, part, P, C, 1e-5, 0.1, 1, None) == EINVAL
    assert L.fpc_batchnorm_bwd(x, y, dy, gamma, stats, dx, dres, dg, db, part, P, C, 0, None) == EINVAL


def test_switch_is_off_when_the_variable_is_unset():
    env = {k: v for k, v in os.environ.items() if k != "FPC_TRAIN_NATIVE_MBV2"}
    code = ("from fastposecnn_amd.lib import train_conv\n"
            "assert train_conv.NATIVE_MBV2 is False\n"
            "assert train_conv._DW_KEEP_TORCH <= {(op, s) for op in ('dgrad', 'wgrad') for s in (1, 2)}\n"
            "assert all(train_conv.counters[k] == 0 for k in %r)\n" % (NEW_KEYS,))
    subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, check=True, timeout=300)
    env["FPC_TRAIN_NATIVE_MBV2"] = "1"
    subprocess.run([sys.executable, "-c", code.replace("is False", "is True")], cwd=REPO, env=env, check=True, timeout=300)


@pytest.mark.parametrize("switch", [False, True])
def test_cpu_tensors_are_torch(monkeypatch, switch):
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_MBV2", switch)
    monkeypatch.setattr(train_conv, "NATIVE_BN", switch)
    monkeypatch.setattr(train_conv, "ENABLED", True)
    torch.manual_seed(0)
    x = torch.randn((2, 32, 6, 5)).contiguous(memory_format=torch.channels_last)
    before = dict(train_conv.counters)
    dw = bb.ConvBNReLU6(32, 32, stride=2, groups=32).train()
    assert [type(m).__name__ for m in dw] == ["Conv2d", "BatchNorm2d", "ReLU6"]
    assert not train_conv._depthwise_ok(x, dw[0].weight, None, 2, 1, 32)
    assert train_conv.batchnorm_act(x, dw[1], relu=False, relu6=True, count_refusal=False) is None
    plain = torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, 2, 1, groups=32, bias=False), torch.nn.BatchNorm2d(32), torch.nn.ReLU6())
    plain.load_state_dict(dw.state_dict())
    with torch.enable_grad():
        y, want = dw(x), plain.train()(x)
    assert torch.equal(y, want)
    y.sum().backward()
    want.sum().backward()
    assert torch.equal(dw[0].weight.grad, plain[0].weight.grad)
    blk = bb.InvertedResidual(32, 32, 1, 6).train()
    assert sorted(blk.state_dict()) == sorted(
        [f"conv.{i}.{j}.{k}" for i in (0, 1) for j, ks in ((0, ["weight"]), (1, ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"])) for k in ks]
        + ["conv.2.weight"] + [f"conv.3.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")])
    blk.eval()          # (BatchNorm on its running statistics: the two calls below see the same module state)
    with torch.enable_grad():
        y = blk(x)
    c = blk.conv
    h = F_relu6(c[0][1](c[0][0](x)))
    h = F_relu6(c[1][1](c[1][0](h)))
    assert torch.equal(y, x + c[3](c[2](h)))
    y.sum().backward()
    assert c[1][0].weight.grad is not None and c[1][0].weight.grad.shape == (192, 1, 3, 3)
    assert dict(train_conv.counters) == before


def F_relu6(t):
    return torch.nn.functional.relu6(t)


@pytest.mark.parametrize("case", R.CASES_ALL, ids=R.ids(R.CASES_ALL))
def test_reference_is_autograd_in_float64(case):
    """The yardstick: the written-out flipped / parity data gradient and the nine-sum weight gradient against torch.autograd.grad
    through F.conv2d(groups = C), float64, on every case of the GPU file."""
    B, Hi, Wi, C, s = case
    for integer in (False, True):
        x, w, dy = R.operands(case, integer)
        assert tuple(dy.shape) == (B, C, *R.out_hw(Hi, Wi, s))
        _, dx, dw = R.autograd_ref(x, w, dy, s)
        got_dx, got_dw = R.dgrad_ref(dy, w, Hi, Wi, s), R.wgrad_ref(x, dy, s)
        assert got_dx.shape == dx.shape and got_dw.shape == dw.shape
        for got, ref, what in ((got_dx, dx, "dx"), (got_dw, dw, "dw")):
            err = (got - ref).abs().max().item()
            assert err <= 1e-12 * max(1.0, ref.abs().max().item()), (what, err)
        if integer:
            assert torch.equal(got_dx, dx) and torch.equal(got_dw, dw)
            assert dx.abs().max().item() < 2 ** 24 and dw.abs().max().item() < 2 ** 24      # exact in f32 too
    if (Hi, Wi) == (1, 1):
        assert (dw.view(C, 9)[:, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all() and dw.view(C, 9)[:, 4].abs().max().item() > 0


def test_relu6_operands_sit_on_both_clamps():
    """What the GPU file's BatchNorm + ReLU6 cases rely on: in float64 more than a fifth of the pre-activations on each clamp,
    and a share within 1e-4 of a kink that is far below the cap of 1e-3."""
    for i, shape in enumerate(R.RELU6_SHAPES):
        x, gy, gamma, beta = R.relu6_operands(i, shape)
        z = torch.nn.functional.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)
        assert (z <= 0).double().mean().item() > 0.2 and (z >= 6).double().mean().item() > 0.2, shape
        near = ((z.abs() <= 1e-4) | ((z - 6).abs() <= 1e-4)).double().mean().item()
        assert near <= 1e-4, (shape, near)
