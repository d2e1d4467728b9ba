"""The three-product form (fpc_conv2d's 6000 + split on k_conv_igemm, 7000 + parts on k_lateral1x1): two fp16 pieces per operand,
A2 B1 + A1 B2 + A1 B1 per 16-deep k group, weights scaled by one power of two per convolution.  Held to the 2e-5 bar of every other convolution form on
the network's own direct shapes, the operand ranges of the fp16-piece forms, and the whole network at the 1e-4 float64 bar."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H3 = 6000            # fpc_conv2d request: 6000 + split-K factor (fused), 6100 + factor (two launches)
LAT_H3 = 7000        # ... 7000 + workgroups per 128-pixel tile: the pixel-resident lateral product on two pieces


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import _native
    _native.lib()
    return L


def _conv2d(dev, x, w, stride, pad, scale=None, shift=None, res=None, up=None, relu=False, bm=0, bn=0, nsplit=H3 + 1):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, Cin, Hi, Wi = x.shape
    Cout, _, Kh, Kw = w.shape
    Ho = (Hi + 2 * pad - Kh) // stride + 1
    Wo = (Wi + 2 * pad - Kw) // stride + 1
    xin = x.permute(0, 2, 3, 1).contiguous().to(dev)
    sb, sh, sw, sc = xin.stride()
    wd = w.contiguous().to(dev)
    out = torch.full((B, Ho, Wo, Cout), float("nan"), device=dev)
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, Ho, Wo, Cin, Cout, Kh, Kw), dtype=torch.uint8, device=dev)
    t = lambda a: None if a is None else a.contiguous().to(dev)
    nhwc = lambda a: None if a is None else a.permute(0, 2, 3, 1).contiguous().to(dev)
    scale_d, shift_d, res_d, up_d = t(scale), t(shift), nhwc(res), nhwc(up)
    nat.check(L.fpc_conv2d(xin.data_ptr(), sb, sh, sw, sc, wd.data_ptr(), nat.ptr(scale_d), nat.ptr(shift_d), nat.ptr(res_d),
                           nat.ptr(up_d), out.data_ptr(), None, B, Hi, Wi, Cin, Cout, Kh, Kw, stride, pad, int(relu), bm, bn, nsplit,
                           ws.data_ptr(), ws.numel(), nat.stream()), "conv2d")
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu()


def _ref(x, w, stride, pad, scale=None, shift=None, res=None, up=None, relu=False):
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if up is not None:
        y = y + F.interpolate(up.double(), scale_factor=2, mode="nearest")
    return y.relu() if relu else y


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


# the network's direct sites at 640 x 480 / 4 (batch 1 here, the same per-image shapes): B, Cin, Hi, Wi, Cout, k, stride, pad, extras,
# (bm, bn, nsplit)
CASES = [
    (1, 64, 120, 160, 128, 3, 2, 1, "bn_relu", (64, 128, H3 + 1)),      # layer2.0 conv1
    (1, 128, 60, 80, 256, 3, 2, 1, "bn_relu", (128, 64, H3 + 1)),       # layer3.0 conv1
    (1, 256, 30, 40, 512, 3, 2, 1, "bn_relu", (64, 128, H3 + 4)),       # layer4.0 conv1, fused split-K
    (1, 256, 30, 40, 512, 3, 2, 1, "bn_relu", (64, 128, H3 + 104)),     # ... split-K summed by k_conv_splitk_epilogue
    (1, 64, 120, 160, 128, 1, 2, 0, "bn", (64, 64, H3 + 1)),            # downsamples
    (1, 128, 60, 80, 256, 1, 2, 0, "bn", (64, 64, H3 + 1)),
    (1, 256, 30, 40, 512, 1, 2, 0, "bn", (64, 128, H3 + 1)),
    (1, 512, 15, 20, 256, 1, 1, 0, "bias", (64, 64, H3 + 1)),           # p5 lateral
    (1, 256, 30, 40, 256, 1, 1, 0, "bias_up", (64, 64, H3 + 1)),        # p4 lateral + up2(p5)
    (1, 128, 60, 80, 256, 1, 1, 0, "bias_up", (128, 128, H3 + 1)),      # p3 lateral + up2(p4), 128 x 128 tiles
    (2, 64, 9, 11, 96, 3, 2, 1, "bias_relu", (64, 64, H3 + 1)),         # ragged: Cout 96, 30 pixels per image
    (1, 96, 13, 17, 40, 3, 1, 1, "bn_relu_res", (128, 64, H3 + 3)),     # ragged Cout 40, split-K
    (1, 96, 13, 17, 42, 3, 1, 1, "bn_relu_res", (64, 64, H3 + 1)),      # Cout 42 (not a multiple of 4): the scalar epilogue
    (2, 64, 7, 9, 42, 1, 2, 0, "bias", (128, 128, H3 + 1)),             # ... 1x1 stride 2, 128 x 128 tiles
    # k_lateral1x1 on two pieces (7000 + parts): K = 64 / 128, bias + top-down addend, ragged pixel tiles, no bias
    (1, 128, 60, 80, 256, 1, 1, 0, "bias_up", (0, 0, LAT_H3 + 8)),      # p3 lateral
    (2, 64, 24, 32, 256, 1, 1, 0, "bias_up", (0, 0, LAT_H3 + 2)),       # p2 lateral shape, K = 64
    (1, 128, 30, 40, 256, 1, 1, 0, "bias", (0, 0, LAT_H3 + 4)),         # 1200 pixels: ragged last tile, no addend
    (3, 64, 10, 14, 96, 1, 1, 0, "bias_relu", (0, 0, LAT_H3 + 3)),      # 140 pixels, Cout 96
    (1, 64, 6, 8, 32, 1, 1, 0, "none", (0, 0, LAT_H3 + 1)),             # no bias
]


def _operands(B, Cin, Hi, Wi, Cout, k, stride, pad, extras, g, xs=1.0, wsc=None):
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    x = torch.randn(B, Cin, Hi, Wi, generator=g) * xs
    if "relu" in extras or "bn" in extras:
        x = x.relu()      # post-ReLU activations as in the network
    w = torch.randn(Cout, Cin, k, k, generator=g) * (wsc if wsc is not None else (2.0 / (Cin * k * k)) ** 0.5)
    kw = {}
    if "bn" in extras:
        kw["scale"] = torch.rand(Cout, generator=g) + 0.5
        kw["shift"] = torch.randn(Cout, generator=g) * 0.1
    if "bias" in extras:
        kw["shift"] = torch.randn(Cout, generator=g) * 0.1
    if "res" in extras:
        kw["res"] = torch.randn(B, Cout, Ho, Wo, generator=g)
    if "up" in extras:
        kw["up"] = torch.randn(B, Cout, Ho // 2, Wo // 2, generator=g)
    kw["relu"] = "relu" in extras
    return x, w, kw


@pytest.mark.parametrize("B,Cin,Hi,Wi,Cout,k,stride,pad,extras,tiling", CASES)
def test_h3_against_float64(lib, dev, B, Cin, Hi, Wi, Cout, k, stride, pad, extras, tiling):
    g = torch.Generator().manual_seed(Cin * 7 + Cout + k)
    x, w, kw = _operands(B, Cin, Hi, Wi, Cout, k, stride, pad, extras, g)
    bm, bn, ns = tiling
    got = _conv2d(dev, x, w, stride, pad, bm=bm, bn=bn, nsplit=ns, **kw)
    ref = _ref(x, w, stride, pad, **kw)
    assert torch.isfinite(got).all()
    assert _rel(got, ref) <= 2e-5


@pytest.mark.parametrize("xs", [1e-2, 1.0, 1e3])
@pytest.mark.parametrize("wsc", [1e-4, 1e-2, 1e2])
def test_h3_operand_ranges(lib, dev, xs, wsc):
    """Activations of scale 1e-2 .. 1e3 and weights of scale 1e-4 .. 1e2 (the power-of-two weight scale absorbs the latter)."""
    g = torch.Generator().manual_seed(11)
    x, w, kw = _operands(1, 128, 30, 40, 256, 3, 2, 1, "bias", g, xs=xs, wsc=wsc)
    kw["shift"] = kw["shift"] * xs * wsc
    got = _conv2d(dev, x, w, 2, 1, **kw)
    assert _rel(got, _ref(x, w, 2, 1, **kw)) <= 2e-5


def test_h3_outlier_stays_finite(lib, dev):
    """A 1e6 activation saturates its fp16 pieces (round toward zero never gives infinity): the output stays finite."""
    g = torch.Generator().manual_seed(5)
    x, w, kw = _operands(1, 64, 24, 32, 128, 3, 2, 1, "bias", g)
    x[0, 3, 5, 7] = 1e6
    got = _conv2d(dev, x, w, 2, 1, **kw)
    assert torch.isfinite(got).all()


def test_h3_repeat_bit_identical(lib, dev):
    g = torch.Generator().manual_seed(3)
    x, w, kw = _operands(1, 256, 30, 40, 512, 3, 2, 1, "bn_relu", g)
    a = _conv2d(dev, x, w, 2, 1, bm=64, bn=128, nsplit=H3 + 4, **kw)
    b = _conv2d(dev, x, w, 2, 1, bm=64, bn=128, nsplit=H3 + 4, **kw)
    assert torch.equal(a, b)


def test_h3_needs_split_level_3(lib, dev):
    """The images are packed only at split level 3: forcing the form below it is refused."""
    from fastposecnn_amd.engine import NetEngine
    m, _ = _model(lib)
    m = m.to(dev)
    eng = NetEngine(m, 1, 64, 96, dev, autotune=False, split_precision=1)
    with pytest.raises(Exception):
        eng.force_direct_h3(1)


def test_h3_plan_codes(lib):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    out = (ctypes.c_int * 4)()
    nat.check(L.fpc_conv2d_plan(1, 60, 80, 128, 256, 3, 3, 128, 64, H3 + 3, out), "plan")
    assert tuple(out)[:3] == (128, 64, 3)
    nat.check(L.fpc_conv2d_plan(1, 60, 80, 128, 256, 3, 3, 64, 64, H3 + 102, out), "plan")
    assert tuple(out)[:3] == (64, 64, 2)


# ---- the network with every candidate site on the form

def _model(lib, seed=0):
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet34"
    hp.PERFORM_AGGREGATION = False
    torch.manual_seed(seed)
    m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
        if isinstance(mod, torch.nn.GroupNorm):
            mod.weight.data.copy_(torch.rand(mod.num_channels, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_channels, generator=g) * 0.1)
    return m.eval(), hp


def _engine(m, B, H, W, dev):
    x = torch.zeros((B, 3, H, W), device=dev)
    with torch.no_grad():
        m(x)
    return m._engines[(B, H, W, x.device)]


def test_network_on_h3_within_1e4_of_float64(lib, dev):
    """ResNet34 with the nine direct sites (3 stride-2 3x3, 3 downsamples, p5 / p4 / p3 laterals) forced onto the form: logits at
    1e-4 of each tensor's scale against the float64 module path; two forwards bit-identical; the p2 fold kept."""
    from fastposecnn_amd import synth
    m, hp = _model(lib)
    x = torch.stack([synth.make_image(i, 64, 96) for i in range(2)])
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp); ref_m.HPARAM.USE_NATIVE_ENGINE = False
    with torch.no_grad():
        ref = ref_m.pure_model_forward(x.double())
    m = m.to(dev)
    eng = _engine(m, 2, 64, 96, dev)
    eng.force_fold(1)
    eng.force_direct_h3(1)
    plans = eng.conv_plans()
    assert sum(1 for p in plans if 6000 <= p[2] < 6200 or 7000 <= p[2] < 8000) == 9 and any(p[2] == 5000 for p in plans)
    with torch.no_grad():
        out = m(x.to(dev))
        out2 = m(x.to(dev))
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = out["logits"][k].cpu().double()
        err = (got - ref[k]).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref[k].abs().max().item()), (k, err)
        assert torch.equal(out["logits"][k], out2["logits"][k]), k
    assert eng.force_direct_h3(0) == 9


def test_network_h3_batch32_graph_replay_bit_equal(lib, dev):
    """ResNet34 at batch 32, 640 x 480, the nine sites on the form: replayed graphs give the plain launches' logits bit for bit."""
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m, _ = _model(lib)
    m = m.to(dev)
    xs = [torch.stack([synth.make_image(i + j) for j in range(32)]).to(dev) for i in range(2)]
    side = torch.cuda.Stream(device=dev)
    runs = []
    for graph in (False, True):
        with torch.no_grad(), torch.cuda.stream(side):
            eng = NetEngine(m, 32, 480, 640, dev, autotune=False, graph=graph, split_precision=3)
            assert eng.force_direct_h3(1) == 9
            outs = []
            for x in xs + xs:
                logits, _ = eng.forward(x)
                outs.append({k: v.clone() for k, v in logits.items()})
        side.synchronize()
        assert eng._lib.fpc_net_graph_recorded(eng._h) == (1 if graph else 0)      # the graph run did replay a recorded graph
        runs.append(outs)
        del eng
    for a, b in zip(*runs):
        for k in a:
            assert torch.equal(a[k], b[k]), k
