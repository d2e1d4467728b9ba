"""CPU-side checks of the EfficientNet depthwise gradient entries (no GPU): the three C ABI additions are declared, listed and
exported and the ABI version did not move; fpc_mbconv_dw_wgrad_workspace_bytes follows include/fpc.h's slice formula; both entries
refuse null and misaligned pointers, bad shapes and a bad workspace before any launch; the float64 references the GPU tests are held
to (_mbconv_train_refs: the kernels' formulas written out) ARE torch.autograd through F.conv2d(F.pad(x, static pads), groups = C)
in float64; and the pads Conv2dStaticSamePadding works out for efficientnet-b0 are the constants the kernels assume at every
depthwise site."""
import ctypes
import os
import re

import pytest
import torch

import _mbconv_train_refs as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
ENTRIES = {      # name -> (result, arguments) as include/fpc.h declares them
    "fpc_mbconv_dw_dgrad": (_i, [_vp] * 3 + [_i] * 6 + [_vp]),
    "fpc_mbconv_dw_wgrad_workspace_bytes": (_sz, [_i] * 5),
    "fpc_mbconv_dw_wgrad": (_i, [_vp] * 3 + [_i] * 6 + [_vp, _sz, _vp]),
}
EINVAL, EWORKSPACE = -1, -2
WALK_LIMIT = 2 ** 32 - 4096 * 256 - 8


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def test_the_three_entries_are_declared_listed_and_exported(hiplib):
    from fastposecnn_amd import _native
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    decl = hdr.index("int fpc_mbconv_dw_dgrad")
    cited = hdr[hdr.rindex("/* ----", 0, decl):decl]      # the block's own comment, from its header to the first declaration
    assert "csrc/depthwise.hip" in cited and cited.count("/*") == 1 and cited.rstrip().endswith("*/")
    assert "F/lib/pose_regressor.py:608-613" in cited and "Conv2dStaticSamePadding(groups = C)" in cited
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
    shapes = [(B, Hi // s, Wi // s, C, k) for B, Hi, Wi, C in R.SHAPES_ALL for k, s in R.KS]
    # the depthwise sites of a 640 x 480 frame at batch 8, and corners
    shapes += [(8, 240, 320, 32, 3), (8, 120, 160, 96, 3), (8, 60, 80, 144, 5), (8, 30, 40, 480, 5), (8, 15, 20, 1152, 5), (8, 15, 20, 1152, 3),
               (1, 1, 1, 4, 5), (1, 1, 300, 4, 5), (64, 1, 1, 2048, 3)]
    for B, Ho, Wo, C, k in shapes:
        n = R.wgrad_slices(B, Ho, Wo, C, k)
        assert 1 <= n <= max(1, min(1024, B * Ho))
        assert L.fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, k) == n * C * k * k * 4, (B, Ho, Wo, C, k)
        if k == 3:      # the count of fpc_dwconv3x3_wgrad: (3, 1) is handed to it with this workspace
            assert L.fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, 3) == L.fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C)
    # where the seams of the GPU file's two extra shapes fall
    B, Hi, Wi, C = R.WGRAD_EXTRA[0]
    assert [R.wgrad_slices(B, Hi // s, Wi // s, C, k) for k, s in R.KS] == [13, 3, 44, 13]
    B, Hi, Wi, C = R.WGRAD_EXTRA[1]
    for k, s in R.KS:
        assert R.wgrad_slices(B, Hi // s, Wi // s, C, k) == 1 and B * (Hi // s) * ((Wi // s + 7) // 8) < 8
    for bad in [(0, 5, 7, 32, 3), (-1, 5, 7, 32, 5), (2, 0, 7, 32, 3), (2, 5, 0, 32, 5), (2, 5, 7, 0, 3), (2, 5, 7, 6, 5), (2, 5, 7, 2, 3),
                (2, 5, 7, -4, 3), (2, 5, 7, 32, 4), (2, 5, 7, 32, 7), (2, 5, 7, 32, 0), (2, 5, 7, 32, 1), (1 << 15, 1 << 10, 1 << 10, 4, 5)]:
        assert L.fpc_mbconv_dw_wgrad_workspace_bytes(*bad) == 0, bad


def _host(n):
    """The address of a 256-byte-aligned host buffer of n floats (validation precedes any launch: it is never dereferenced)."""
    buf = ctypes.create_string_buffer(4 * n + 256)
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 256


def test_depthwise_refusals_come_before_any_launch(hiplib):
    L = hiplib
    B, H, W, C = 2, 6, 8, 32
    keep = []

    def p(n):
        buf, a = _host(n)
        keep.append(buf)
        return a
    big = B * H * W * C
    need = max(L.fpc_mbconv_dw_wgrad_workspace_bytes(B, H, W, C, k) for k in (3, 5))
    assert need > 0
    wsp = p(need // 4)
    dgrad = lambda ptrs, B_=B, H_=H, W_=W, C_=C, k=5, s=1: L.fpc_mbconv_dw_dgrad(*ptrs, B_, H_, W_, C_, k, s, None)
    wgrad = lambda ptrs, B_=B, H_=H, W_=W, C_=C, k=5, s=1, ws=None, nb=need: L.fpc_mbconv_dw_wgrad(*ptrs, B_, H_, W_, C_, k, s, ws or wsp, nb, None)
    for fn, good in ((dgrad, [p(big), p(25 * C), p(big)]), (wgrad, [p(big), p(big), p(25 * C)])):
        for k, s in R.KS:
            for i in range(3):
                args = list(good)
                args[i] = good[i] + 4
                assert fn(args, k=k, s=s) == EINVAL, ("misaligned", i)
                args[i] = None
                assert fn(args, k=k, s=s) == EINVAL, ("null", i)
            for B_bad in (0, -2):
                assert fn(good, B_=B_bad, k=k, s=s) == EINVAL
            for C_bad in (0, 2, 6, -4, 30):
                assert fn(good, C_=C_bad, k=k, s=s) == EINVAL, C_bad
            assert fn(good, H_=0, k=k, s=s) == EINVAL and fn(good, W_=0, k=k, s=s) == EINVAL and fn(good, H_=-2, k=k, s=s) == EINVAL
            # an item count past the 32-bit walk limit: B Hi Wi C / 4 quads
            assert (1 << 11) * (1 << 11) * (1 << 10) * 1 >= WALK_LIMIT
            assert fn(good, B_=1 << 10, H_=1 << 11, W_=1 << 11, C_=4, k=k, s=s) == EINVAL
        for k_bad in (0, 1, 2, 4, 7, -3):
            assert fn(good, k=k_bad) == EINVAL and fn(good, k=k_bad, s=2) == EINVAL, k_bad
        for s_bad in (0, 3, -1, 4):
            assert fn(good, k=3, s=s_bad) == EINVAL and fn(good, k=5, s=s_bad) == EINVAL, s_bad
        for k in (3, 5):      # an odd extent at stride 2, as fpc_mbconv_dw refuses it
            assert fn(good, H_=5, k=k, s=2) == EINVAL and fn(good, W_=7, k=k, s=2) == EINVAL and fn(good, H_=5, W_=7, k=k, s=2) == EINVAL
    wgood = [p(big), p(big), p(25 * C)]
    for k, s in R.KS:
        need_k = L.fpc_mbconv_dw_wgrad_workspace_bytes(B, H // s, W // s, C, k)
        assert L.fpc_mbconv_dw_wgrad(*wgood, B, H, W, C, k, s, None, need, None) == EINVAL             # a null workspace
        assert wgrad(wgood, k=k, s=s, ws=wsp + 16) == EWORKSPACE                                        # not 256-byte aligned
        assert wgrad(wgood, k=k, s=s, nb=need_k - 1) == EWORKSPACE and wgrad(wgood, k=k, s=s, nb=0) == EWORKSPACE      # too small


@pytest.mark.parametrize("ks", R.KS, ids=str)
def test_reference_is_autograd_in_float64(ks):
    """The yardstick: the written-out flipped / parity data gradient and the k k sums of the weight gradient against
    torch.autograd.grad through F.conv2d(F.pad(x, static pads), groups = C), float64, on every shape of the GPU file.  It pins the
    reference, not the kernels: it passes without csrc/depthwise.hip too (the entry, refusal, workspace and GPU tests do not)."""
    k, s = ks
    for shape in R.SHAPES_ALL:
        B, Hi, Wi, C = shape
        for integer in (False, True):
            x, w, dy = R.operands(shape, k, s, integer)
            y, dx, dw = R.autograd_ref(x, w, dy, k, s)
            assert tuple(y.shape) == tuple(dy.shape) == (B, C, Hi // s, Wi // s)
            got_dx, got_dw = R.dgrad_ref(dy, w, Hi, Wi, k, s), R.wgrad_ref(x, dy, k, s)
            assert got_dx.shape == dx.shape and got_dw.shape == dw.shape
            for got, ref, what in ((got_dx, dx, "dx"), (got_dw, dw, "dw")):
                err = (got - ref).abs().max().item()
                assert err <= 1e-12 * max(1.0, ref.abs().max().item()), (what, shape, err)
            if integer:
                assert torch.equal(got_dx, dx) and torch.equal(got_dw, dw)
                assert dx.abs().max().item() < 2 ** 24 and dw.abs().max().item() < 2 ** 24      # exact in f32 too
        if (Hi, Wi, k, s) == (2, 2, 5, 1):      # the 16 taps no pixel of a 2 x 2 map reaches
            flat = dw.view(C, 5, 5)
            reached = torch.zeros((5, 5), dtype=torch.bool)
            reached[1:4, 1:4] = True
            assert int((~reached).sum()) == 16 and (flat[:, ~reached] == 0).all() and (flat[:, reached] != 0).any()


def test_static_pads_of_b0_are_the_kernels_constants():
    """The module's pads at the 16 depthwise sites against the references' (which are the kernels' compile-time constants).  It
    pins what the kernels may assume about the module, not the kernels: it passes without csrc/depthwise.hip too."""
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder("efficientnet-b0")
    sites = [b._depthwise_conv for b in enc._blocks]
    assert len(sites) == 16 and sum(c.kernel_size == (5, 5) for c in sites) == 9
    seen = set()
    for conv in sites:
        k, s = conv.kernel_size[0], conv.stride[0]
        before, after = R.pads(k, s)
        assert isinstance(conv.static_padding, torch.nn.ZeroPad2d) and tuple(conv.static_padding.padding) == (before, after, before, after)
        assert conv.groups == conv.in_channels == conv.out_channels and conv.bias is None and conv.in_channels % 4 == 0
        seen.add((k, s))
    assert seen == set(R.KS)
    assert [R.pads(k, s) for k, s in R.KS] == [(1, 1), (0, 1), (2, 2), (1, 2)]
