"""The training-side kernels of the grouped 3x3 convolution (csrc/conv_grouped_train.hip) on the MI355X through the C ABI,
fpc_conv2d_grouped_dgrad and fpc_conv2d_grouped_wgrad, against float64 conv2d(groups=32) autograd on the CPU at the project's
bars: dx within 2e-5 max(1, |ref|max), dw within 1e-4 max(1, |ref|max).  The shapes are test_gpu_conv_grouped.py's CASES (the
smallest at which tiles, seams and borders can go wrong) plus one whose tile count the weight gradient's slices do not divide.
Outputs are prefilled with NaN; two calls give identical bits; small integers are exact; groups do not mix; refusals launch
nothing."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GROUPS = 32

# name: (B, H, W, C, Cg, stride) — test_gpu_conv_grouped.py::CASES
CASES = {
    "a": (2, 24, 40, 128, 4, 1),         # several tiles, frame seam; 18 tiles in 18 slices
    "b": (1, 3, 5, 128, 4, 1),           # a map that is all border: fewer pixels than one slice
    "c": (1, 25, 37, 256, 8, 2),         # odd input -> 13 x 19
    "d": (1, 26, 38, 256, 8, 2),         # even input
    "e": (3, 16, 20, 512, 16, 1),        # 12 tiles in 3 slices
    "f": (2, 15, 20, 1024, 32, 1),
    "g": (1, 30, 40, 1024, 32, 2),
    "h_f": (2, 15, 20, 2048, 64, 1),     # Cg = 64 twins of f and g
    "h_g": (1, 30, 40, 2048, 64, 2),
}
# the weight gradient's slice seams: 5 tiles of 8 x 16 in 2 slices (2 + 3 tiles)
SEAM = {"s": (1, 8, 80, 512, 16, 1)}
ALL = dict(CASES, **SEAM)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _tiles(B, Ho, Wo, stride):
    return B * ((Ho + 7) // 8) * ((Wo + (16 if stride == 1 else 8) - 1) // (16 if stride == 1 else 8))


def _slices(L, B, Ho, Wo, C, groups, stride):
    """The slice count of a weight-gradient call, from the workspace size as include/fpc.h documents it."""
    by = L.fpc_conv2d_grouped_wgrad_workspace_bytes(B, Ho, Wo, C, groups)
    per = C * (C // groups) * 36
    assert by > 0 and by % per == 0
    return min(by // per, _tiles(B, Ho, Wo, stride))


def _dgrad(dev, dy, w, H, W, stride, groups=GROUPS, ws_short=0, dy_offset=0):
    """fpc_conv2d_grouped_dgrad; dy NCHW on the CPU -> (rc, dx NCHW on the CPU; NaN where nothing was written)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, C = dy.shape[:2]
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(dev)
    if dy_offset:
        buf = torch.empty(dyd.numel() + dy_offset, device=dev)
        buf[dy_offset:] = dyd.reshape(-1)
        dyd = buf[dy_offset:]
    wd = w.contiguous().to(dev)
    dx = torch.full((B, H, W, C), float("nan"), device=dev)
    n = max(L.fpc_conv2d_grouped_dgrad_workspace_bytes(C, groups), 256)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = L.fpc_conv2d_grouped_dgrad(dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, H, W, C, groups, stride, ws.data_ptr(),
                                    n - ws_short, nat.stream())
    torch.cuda.synchronize()
    return rc, dx.permute(0, 3, 1, 2).cpu()


def _wgrad(dev, x, dy, stride, groups=GROUPS, ws_short=0, wide=0, nhwc_input=True, cg=None):
    """fpc_conv2d_grouped_wgrad; x, dy NCHW on the CPU -> (rc, dw OIHW on the CPU; NaN where nothing was written).  wide > 0: x is
    the first C channels of a tensor of C + wide channels (sw = C + wide)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, C, H, W = x.shape
    Ho, Wo = _out_hw(H, W, stride)
    if nhwc_input:
        full = torch.randn((B, H, W, C + wide), generator=torch.Generator().manual_seed(5)).to(dev)
        full[..., :C] = x.permute(0, 2, 3, 1).to(dev)
        xd = full[..., :C]
        sb, sh, sw, sc = xd.stride()
        assert sc == 1 and sw == C + wide
    else:
        xd = x.contiguous().to(dev)      # NCHW: the entry has no channel stride, the pixel stride it is given is wrong on purpose
        sb, _, sh, sw = xd.stride()
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(dev)
    cg = cg if cg is not None else (C // groups if groups and C % groups == 0 else 4)
    dw = torch.full((C, cg, 3, 3), float("nan"), device=dev)
    n = max(L.fpc_conv2d_grouped_wgrad_workspace_bytes(B, Ho, Wo, C, groups), 256)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = L.fpc_conv2d_grouped_wgrad(xd.data_ptr(), sb, sh, sw, dyd.data_ptr(), dw.data_ptr(), B, H, W, C, groups, stride,
                                    ws.data_ptr(), n - ws_short, nat.stream())
    torch.cuda.synchronize()
    return rc, dw.cpu()


def _refs(x, w, dy, stride):
    """float64 autograd of conv2d(groups=32) on the CPU: (dx, dw)."""
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, stride, 1, 1, GROUPS).backward(dy.double())
    return xr.grad, wr.grad


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands and the float64 references of a case, computed once: (x, w, dy, dx ref, dw ref)."""
    B, H, W, C, Cg, stride = ALL[name]
    assert C == GROUPS * Cg
    Ho, Wo = _out_hw(H, W, stride)
    g = torch.Generator().manual_seed(100 + sorted(ALL).index(name))
    x = torch.randn((B, C, H, W), generator=g)
    w = torch.randn((C, Cg, 3, 3), generator=g) / (9 * Cg) ** 0.5
    dy = torch.randn((B, C, Ho, Wo), generator=g)
    dx, dw = _refs(x, w, dy, stride)
    return x, w, dy, dx, dw


@pytest.mark.parametrize("name", sorted(CASES))
def test_dgrad_vs_float64(dev, name):
    x, w, dy, ref, _ = _case(name)
    _, H, W, _, _, stride = ALL[name]
    rc, out = _dgrad(dev, dy, w, H, W, stride)
    assert rc == 0
    assert out.shape == ref.shape
    assert not torch.isnan(out).any(), "unwritten outputs"
    err = (out.double() - ref).abs().max().item()
    print(f"dgrad case {name}: err {err:.3e} |ref|max {ref.abs().max().item():.3f}")
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err
    rc2, out2 = _dgrad(dev, dy, w, H, W, stride)
    assert rc2 == 0 and torch.equal(out, out2)              # two calls: identical bits


@pytest.mark.parametrize("name", sorted(ALL))
def test_wgrad_vs_float64(dev, name):
    x, w, dy, _, ref = _case(name)
    stride = ALL[name][5]
    rc, out = _wgrad(dev, x, dy, stride)
    assert rc == 0
    assert out.shape == ref.shape
    assert not torch.isnan(out).any(), "unwritten outputs"
    err = (out.double() - ref).abs().max().item()
    print(f"wgrad case {name}: err {err:.3e} |ref|max {ref.abs().max().item():.3f}")
    assert err <= 1e-4 * max(1.0, ref.abs().max().item()), err
    rc2, out2 = _wgrad(dev, x, dy, stride)
    assert rc2 == 0 and torch.equal(out, out2)              # two calls: identical bits


def test_wgrad_slice_seams_are_covered(dev):
    """The cases of test_wgrad_vs_float64 hold the three slice situations: a tile count the slice count does not divide, a map
    smaller than one slice, and several slices (the reduce kernel runs)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    n = {}
    for name, (B, H, W, C, Cg, stride) in ALL.items():
        Ho, Wo = _out_hw(H, W, stride)
        n[name] = (_tiles(B, Ho, Wo, stride), _slices(L, B, Ho, Wo, C, GROUPS, stride))
    print(n)
    assert n["s"][1] > 1 and n["s"][0] % n["s"][1] != 0           # uneven slices
    assert n["b"] == (1, 1)                                       # one tile of 15 pixels, one slice, no reduce
    assert n["a"][1] > 1 and n["e"][1] > 1 and n["e"][0] > n["e"][1]      # several slices, several tiles per slice


@pytest.mark.parametrize("name", ["a", "c", "e", "g", "h_f"])
def test_small_integers_are_exact(dev, name):
    """|x| <= 8, |dy| <= 4, |w| <= 4 integers.  dx sums at most 9 * 64 products of magnitude <= 16, dw at most 1 920 pixels of
    magnitude <= 32 (case a): every partial sum is an integer below 2^24, so both must equal float64 bit for bit.  This pins the
    tap and parity indexing the tolerance tests could blur."""
    B, H, W, C, Cg, stride = CASES[name]
    Ho, Wo = _out_hw(H, W, stride)
    g = torch.Generator().manual_seed(77)
    x = torch.randint(-8, 9, (B, C, H, W), generator=g).float()
    w = torch.randint(-4, 5, (C, Cg, 3, 3), generator=g).float()
    dy = torch.randint(-4, 5, (B, C, Ho, Wo), generator=g).float()
    rdx, rdw = _refs(x, w, dy, stride)
    rc, dx = _dgrad(dev, dy, w, H, W, stride)
    assert rc == 0 and torch.equal(dx.double(), rdx)
    rc, dw = _wgrad(dev, x, dy, stride)
    assert rc == 0 and torch.equal(dw.double(), rdw)


@pytest.mark.parametrize("name,group", [(n, g) for n in ("a", "d", "f", "h_g") for g in (0, 13, 31)])
def test_group_isolation(dev, name, group):
    """dy zero outside one group's channels: dx and dw are exactly 0.0 outside that group, and right inside it."""
    x, w, dy, _, _ = _case(name)
    _, H, W, C, Cg, stride = CASES[name]
    dz = torch.zeros_like(dy)
    dz[:, group * Cg:(group + 1) * Cg] = dy[:, group * Cg:(group + 1) * Cg]
    rdx, rdw = _refs(x, w, dz, stride)
    inside = torch.zeros(C, dtype=torch.bool)
    inside[group * Cg:(group + 1) * Cg] = True
    rc, dx = _dgrad(dev, dz, w, H, W, stride)
    assert rc == 0 and (dx[:, ~inside] == 0.0).all()
    assert (dx[:, inside].double() - rdx[:, inside]).abs().max().item() <= 2e-5 * max(1.0, rdx.abs().max().item())
    assert dx[:, inside].abs().max().item() > 0.0
    rc, dw = _wgrad(dev, x, dz, stride)
    assert rc == 0 and (dw[~inside] == 0.0).all()
    assert (dw[inside].double() - rdw[inside]).abs().max().item() <= 1e-4 * max(1.0, rdw.abs().max().item())
    assert dw[inside].abs().max().item() > 0.0


@pytest.mark.parametrize("name", ["a", "d"])
def test_wgrad_of_a_strided_view(dev, name):
    """x as a channel slice of a wider NHWC tensor (C of C + 32 channels, sw = C + 32; case a: 128 of 160): the other channels, random,
    are never read."""
    x, w, dy, _, ref = _case(name)
    stride = CASES[name][5]
    rc, out = _wgrad(dev, x, dy, stride, wide=32)
    assert rc == 0 and not torch.isnan(out).any()
    assert (out.double() - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
    rc0, dense = _wgrad(dev, x, dy, stride)
    assert rc0 == 0 and torch.equal(out, dense)


def test_refusals_launch_nothing(dev):
    """The refusal list of test_gpu_conv_grouped.py::test_refusals_launch_nothing on both entries, a workspace one byte short and
    misaligned pointers: FPC_EINVAL, the outputs stay all NaN, the workspace size of a refused shape is 0."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    g = torch.Generator().manual_seed(3)

    def run(C, Cg, groups, stride=1, **kw):
        H, W = 6, 7
        Ho, Wo = _out_hw(H, W, stride if stride in (1, 2) else 1)
        x = torch.randn((1, C, H, W), generator=g)
        w = torch.randn((C, Cg, 3, 3), generator=g)
        dy = torch.randn((1, C, Ho, Wo), generator=g)
        dkw = {k: v for k, v in kw.items() if k in ("ws_short", "dy_offset")}
        wkw = {k: v for k, v in kw.items() if k in ("ws_short", "nhwc_input")}
        rcd, dx = _dgrad(dev, dy, w, H, W, stride, groups=groups, **dkw)
        rcw, dw = _wgrad(dev, x, dy, stride, groups=groups, cg=Cg, **wkw)
        return (rcd, bool(torch.isnan(dx).all())), (rcw, bool(torch.isnan(dw).all()))

    ok, bad = (0, False), (-1, True)
    assert run(128, 4, 32) == (ok, ok)                                # the control: this one runs
    assert run(128, 4, 32, stride=2) == (ok, ok)
    assert run(128, 4, 24) == (bad, bad)                              # groups not dividing the width
    assert run(128, 2, 64) == (bad, bad)                              # Cg = 2
    assert run(128, 128, 1) == (bad, bad)                             # Cg = 128 (a dense convolution)
    assert run(48, 4, 12) == (bad, bad)                               # C not a multiple of 32
    assert run(128, 4, 32, stride=3) == (bad, bad)
    assert run(128, 4, 32, ws_short=1) == (bad, bad)                  # a workspace one byte short
    assert run(128, 4, 32, nhwc_input=False)[1] == bad                # x with a channel stride != 1: its pixel stride is 1 < C
    assert run(128, 4, 32, dy_offset=1)[0] == bad                     # dy 4 bytes off a 16-byte boundary
    for C, groups in ((128, 24), (128, 64), (128, 1), (48, 12)):
        assert L.fpc_conv2d_grouped_dgrad_workspace_bytes(C, groups) == 0
        assert L.fpc_conv2d_grouped_wgrad_workspace_bytes(1, 6, 7, C, groups) == 0
    # null pointers
    dy = torch.randn((1, 6, 7, 128), generator=g).to(dev)
    w = torch.randn((128, 4, 3, 3), generator=g).to(dev)
    dx = torch.full((1, 6, 7, 128), float("nan"), device=dev)
    dw = torch.full((128, 4, 3, 3), float("nan"), device=dev)
    ws = torch.empty(max(L.fpc_conv2d_grouped_dgrad_workspace_bytes(128, 32), L.fpc_conv2d_grouped_wgrad_workspace_bytes(1, 6, 7, 128, 32)),
                     dtype=torch.uint8, device=dev)
    s = nat.stream()
    for args in ((None, w.data_ptr(), dx.data_ptr()), (dy.data_ptr(), None, dx.data_ptr()), (dy.data_ptr(), w.data_ptr(), None)):
        assert L.fpc_conv2d_grouped_dgrad(*args, 1, 6, 7, 128, 32, 1, ws.data_ptr(), ws.numel(), s) == -1
    assert L.fpc_conv2d_grouped_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), 1, 6, 7, 128, 32, 1, None, ws.numel(), s) == -1
    st = (6 * 7 * 128, 7 * 128, 128)
    for args in ((None, *st, dy.data_ptr(), dw.data_ptr()), (dy.data_ptr(), *st, None, dw.data_ptr()), (dy.data_ptr(), *st, dy.data_ptr(), None)):
        assert L.fpc_conv2d_grouped_wgrad(*args, 1, 6, 7, 128, 32, 1, ws.data_ptr(), ws.numel(), s) == -1
    assert L.fpc_conv2d_grouped_wgrad(dy.data_ptr(), *st, dy.data_ptr(), dw.data_ptr(), 1, 6, 7, 128, 32, 1, None, ws.numel(), s) == -1
    assert L.fpc_conv2d_grouped_wgrad(dy.data_ptr(), 6 * 7 * 128, 7 * 128, 130, dy.data_ptr(), dw.data_ptr(), 1, 6, 7, 128, 32, 1,
                                      ws.data_ptr(), ws.numel(), s) == -1      # a pixel stride that is not a multiple of 4
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(dw).all())
