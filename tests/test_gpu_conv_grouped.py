"""k_conv3x3_grouped (csrc/conv_grouped.hip) on the MI355X through fpc_conv2d_grouped, against float64 conv2d(groups=32) on the
CPU at the project's convolution bar, err <= 2e-5 max(1, |ref|max): every case with every form built, each with and without
scale / shift + ReLU; group isolation; bit-exact results on small integers; run-to-run identity; refusals."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FORMS = [0]          # the forms built: 0 = plain f32 products
GROUPS = 32

# name: (B, H, W, C, Cg, stride)
CASES = {
    "a": (2, 24, 40, 128, 4, 1),         # several tiles, frame seam
    "b": (1, 3, 5, 128, 4, 1),           # a map that is all border
    "c": (1, 25, 37, 256, 8, 2),         # odd input -> 13 x 19: the right / bottom padding taps are read
    "d": (1, 26, 38, 256, 8, 2),         # even input
    "e": (3, 16, 20, 512, 16, 1),
    "f": (2, 15, 20, 1024, 32, 1),       # the network's own smallest map
    "g": (1, 30, 40, 1024, 32, 2),       # -> 15 x 20
    "h_f": (2, 15, 20, 2048, 64, 1),     # Cg = 64 twins of f and g (resnext101_32x8d's layer4)
    "h_g": (1, 30, 40, 2048, 64, 2),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _grouped(dev, x, w, stride, form=0, scale=None, shift=None, relu=False, groups=GROUPS, nhwc_input=True):
    """fpc_conv2d_grouped; x NCHW on the CPU -> (rc, out NCHW on the CPU; NaN where nothing was written)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, C, Hi, Wi = x.shape
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    if nhwc_input:
        xin = x.permute(0, 2, 3, 1).contiguous().to(dev)
        sb, sh, sw, sc = xin.stride()
    else:
        xin = x.contiguous().to(dev)
        sb, sc, sh, sw = xin.stride()
    wd = w.contiguous().to(dev)
    t = lambda a: None if a is None else a.contiguous().to(dev)
    scale_d, shift_d = t(scale), t(shift)
    out = torch.full((B, Ho, Wo, C), float("nan"), device=dev)
    ws = torch.empty(max(L.fpc_conv2d_grouped_workspace_bytes(C, groups), 256), dtype=torch.uint8, device=dev)
    rc = L.fpc_conv2d_grouped(xin.data_ptr(), sb, sh, sw, sc, wd.data_ptr(), nat.ptr(scale_d), nat.ptr(shift_d), out.data_ptr(),
                              B, Hi, Wi, C, groups, stride, int(relu), form, ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    return rc, out.permute(0, 3, 1, 2).cpu()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands and the float64 references of a case, computed once: (x, w, scale, shift, ref plain, ref with BN + ReLU)."""
    B, H, W, C, Cg, stride = CASES[name]
    assert C == GROUPS * Cg
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    x = torch.randn((B, C, H, W), generator=g)
    w = torch.randn((C, Cg, 3, 3), generator=g) / (9 * Cg) ** 0.5
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, stride, 1, 1, GROUPS)
    ref_bn = (ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).relu()
    return x, w, scale, shift, ref, ref_bn


@pytest.mark.parametrize("epilogue", ["plain", "bn_relu"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_vs_float64(dev, name, form, epilogue):
    x, w, scale, shift, ref, ref_bn = _case(name)
    stride = CASES[name][5]
    kw = dict(scale=scale, shift=shift, relu=True) if epilogue == "bn_relu" else {}
    want = ref_bn if epilogue == "bn_relu" else ref
    rc, out = _grouped(dev, x, w, stride, form, **kw)
    assert rc == 0
    assert out.shape == want.shape
    assert not torch.isnan(out).any(), "unwritten outputs"
    err = (out.double() - want).abs().max().item()
    print(f"case {name} form {form} {epilogue}: err {err:.3e} |ref|max {want.abs().max().item():.3f}")
    assert err <= 2e-5 * max(1.0, want.abs().max().item()), err
    rc2, out2 = _grouped(dev, x, w, stride, form, **kw)
    assert rc2 == 0 and torch.equal(out, out2)              # two calls: identical bits


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,group", [(n, g) for n in ("a", "d", "f", "h_g") for g in (0, 13, 31)])
def test_group_isolation(dev, name, form, group):
    """Input zero outside one group's channels, scale but no shift: every output channel outside that group is exactly 0.0."""
    x, w, scale, _, _, _ = _case(name)
    Cg, stride = CASES[name][4], CASES[name][5]
    xz = torch.zeros_like(x)
    xz[:, group * Cg:(group + 1) * Cg] = x[:, group * Cg:(group + 1) * Cg]
    rc, out = _grouped(dev, xz, w, stride, form, scale=scale)
    assert rc == 0
    inside = torch.zeros(x.shape[1], dtype=torch.bool)
    inside[group * Cg:(group + 1) * Cg] = True
    assert (out[:, ~inside] == 0.0).all()
    ref = F.conv2d(xz.double(), w.double(), None, stride, 1, 1, GROUPS) * scale.double().view(1, -1, 1, 1)
    assert (out[:, inside].double() - ref[:, inside]).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    assert out[:, inside].abs().max().item() > 0.0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["a", "c", "e", "g", "h_f"])
def test_small_integers_are_exact(dev, name, form):
    """|x| <= 8, |w| <= 4 integers: every product and partial sum is an integer below 2^24 (9 * 64 * 32 = 18 432 at most), so the
    f32 chain — and a bf16 x 3 split of such operands — gives the float64 result bit for bit."""
    B, H, W, C, Cg, stride = CASES[name]
    g = torch.Generator().manual_seed(77)
    x = torch.randint(-8, 9, (B, C, H, W), generator=g).float()
    w = torch.randint(-4, 5, (C, Cg, 3, 3), generator=g).float()
    rc, out = _grouped(dev, x, w, stride, form)
    assert rc == 0
    ref = F.conv2d(x.double(), w.double(), None, stride, 1, 1, GROUPS)
    assert torch.equal(out.double(), ref)


def test_refusals_launch_nothing(dev):
    g = torch.Generator().manual_seed(3)
    def run(C, Cg, groups, stride=1, form=0, **kw):
        x = torch.randn((1, C, 6, 7), generator=g)
        w = torch.randn((C, Cg, 3, 3), generator=g)
        rc, out = _grouped(dev, x, w, stride, form, groups=groups, **kw)
        return rc, bool(torch.isnan(out).all())
    assert run(128, 4, 32) == (0, False)                          # the control: this one runs
    assert run(128, 4, 24) == (-1, True)                          # groups not dividing the width
    assert run(128, 2, 64) == (-1, True)                          # Cg = 2
    assert run(128, 128, 1) == (-1, True)                         # Cg = 128 (a dense convolution: fpc_conv2d)
    assert run(48, 4, 12) == (-1, True)                           # C not a multiple of 32
    assert run(128, 4, 32, stride=3) == (-1, True)
    assert run(128, 4, 32, form=1) == (-1, True)                  # a form that is not built
    assert run(128, 4, 32, form=-1) == (-1, True)
    assert run(128, 4, 32, nhwc_input=False) == (-1, True)        # channel stride != 1
    # the dense entry has no groups: it refuses the grouped plan code
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    x = torch.randn((1, 8, 8, 128), generator=g).to(dev)
    w = torch.randn((128, 128, 3, 3), generator=g).to(dev)
    out = torch.full((1, 8, 8, 128), float("nan"), device=dev)
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(1, 8, 8, 128, 128, 3, 3), dtype=torch.uint8, device=dev)
    sb, sh, sw, sc = x.stride()
    rc = L.fpc_conv2d(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), None, None, None, None, out.data_ptr(), None, 1, 8, 8, 128, 128,
                      3, 3, 1, 1, 0, 0, 0, 8000, ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(out).all())
