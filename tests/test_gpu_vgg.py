"""GPU checks of the VGG encoders: the two kernels of csrc/vgg.hip against float64 (whole numbers and a one-hot pixel bit for bit, NaN
in the image's ignored channel, patterns around every output, two launches the same bits), four engines (all six feature levels and
every logit at the network bar, the wino-eligible sites on a Winograd form), graph replay and the streamer bit for bit against the
eager forward, and one training step."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _vgg_model as V
from _densenet_kernels import NAN, _bar, _twice

pytestmark = pytest.mark.gpu

# one pixel; under one workgroup step of 16 pixels; frames that straddle workgroup steps; odd sizes over several steps; several
# workgroups of a grid rounded to the XCD bands (9216 pixels: 36 -> 40 workgroups, the banded walk)
CONV_SHAPES = [(1, 1, 1), (1, 2, 3), (2, 5, 7), (1, 33, 65), (3, 32, 96)]
POOL_SHAPES = [(1, 2, 2, 4), (2, 6, 10, 64), (1, 34, 66, 512), (3, 2, 2, 12)]


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


# -------------------------------------------------------------------------------------------------------------- fpc_conv3x3_c3

def _c3_run(dev, x, w, scale, shift, act):
    """x [B][3][H][W] -> the kernel's out as [B][64][H][W]; the image's fourth channel is NaN."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, _, H, W = x.shape
    x4 = torch.full((B, H, W, 4), NAN)
    x4[..., :3] = x.permute(0, 2, 3, 1)
    xd, wd, td = x4.to(dev), w.contiguous().to(dev), shift.to(dev)
    sd = scale.to(dev) if scale is not None else None
    out = _twice(dev, torch.full((B * H * W * 64,), NAN), lambda y: L.fpc_conv3x3_c3(
        xd.data_ptr(), wd.data_ptr(), sd.data_ptr() if sd is not None else None, td.data_ptr(), y, B, H, W, 64, act, nat.stream()))
    assert torch.isfinite(out).all(), "the image's fourth channel reached the output"
    return out.view(B, H, W, 64).permute(0, 3, 1, 2)


def _c3_ref(x, w, scale, shift, act):
    v = F.conv2d(x.double(), w.double(), None, 1, 1)
    if scale is not None:
        v = v * scale.double().view(1, -1, 1, 1)
    v = v + shift.double().view(1, -1, 1, 1)
    return v.clamp_min(0.0) if act else v


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("aff", [True, False], ids=["scale", "bias"])
@pytest.mark.parametrize("B,H,W", CONV_SHAPES)
def test_conv3x3_c3_vs_float64(lib, dev, B, H, W, aff, act):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + act)
    x = torch.randn((B, 3, H, W), generator=g)
    w = torch.randn((64, 3, 3, 3), generator=g) * (2.0 / 27) ** 0.5
    scale = torch.rand(64, generator=g) + 0.5 if aff else None
    shift = torch.randn(64, generator=g) * 0.5
    out = _c3_run(dev, x, w, scale, shift, act)
    _bar(out, _c3_ref(x, w, scale, shift, act), f"conv3x3_c3 {(B, H, W)} aff{aff} act{act}")
    assert (out.min() >= 0.0) if act else (out.min() < 0.0)


@pytest.mark.parametrize("aff", [True, False], ids=["scale", "bias"])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 33, 65)])
def test_conv3x3_c3_whole_numbers_bit_for_bit(lib, dev, B, H, W, aff):
    g = torch.Generator().manual_seed(H + W)
    x = torch.randint(-4, 5, (B, 3, H, W), generator=g).float()
    w = torch.randint(-2, 3, (64, 3, 3, 3), generator=g).float()
    scale = torch.randint(1, 4, (64,), generator=g).float() if aff else None
    shift = torch.randint(-5, 6, (64,), generator=g).float()
    for act in (0, 1):
        assert torch.equal(_c3_run(dev, x, w, scale, shift, act).double(), _c3_ref(x, w, scale, shift, act)), act


def test_conv3x3_c3_one_hot_pixel_at_each_corner(lib, dev):
    """A single 1 at a corner returns the flipped taps that lie inside the image, bit for bit, and exact zeros elsewhere: every tap
    and the padding select."""
    g = torch.Generator().manual_seed(11)
    w = torch.randn((64, 3, 3, 3), generator=g)
    B, H, W = 2, 4, 5
    for k, (h0, w0) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        x = torch.zeros((B, 3, H, W))
        x[k % B, k % 3, h0, w0] = 1.0
        out = _c3_run(dev, x, w, None, torch.zeros(64), 0)
        want = torch.zeros((B, 64, H, W))
        for kh in range(3):
            for kw in range(3):
                h, ww = h0 + 1 - kh, w0 + 1 - kw
                if 0 <= h < H and 0 <= ww < W:
                    want[k % B, :, h, ww] = w[:, k % 3, kh, kw]
        assert torch.equal(out, want), (h0, w0)
        assert torch.equal(out.double(), _c3_ref(x, w, None, torch.zeros(64), 0))


# ---------------------------------------------------------------------------------------------------------- fpc_maxpool2x2_fwd

@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_maxpool2x2(lib, dev, B, H, W, C):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    x = torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(H * W + C))
    xd = x.to(dev)
    out = _twice(dev, torch.full((B * (H // 2) * (W // 2) * C,), NAN),
                 lambda y: L.fpc_maxpool2x2_fwd(xd.data_ptr(), y, B, H, W, C, nat.stream())).view(B, H // 2, W // 2, C)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(out.view(torch.int32), want.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the engines

_REFS = {}


def _float64(lib, encoder, B, H, W):
    """(model, hp, x, float64 logits, float64 encoder features), computed once per configuration and left unchanged."""
    key = (encoder, B, H, W)
    if key not in _REFS:
        m, hp = V.model(lib, encoder)      # (the draw tests/test_vgg_encoder.py holds to a quarter of the network bar in torch's own f32)
        x = V.images(B, H, W)
        ref_m = copy.deepcopy(m).double()
        ref_m.HPARAM = copy.copy(hp)
        ref_m.HPARAM.USE_NATIVE_ENGINE = False
        with torch.no_grad():
            _REFS[key] = (m, hp, x, ref_m.pure_model_forward(x.double()), ref_m.encoder(x.double()))
    return _REFS[key]


def _check(eng, logits, ref, feats, what, tol=1e-4):
    """All six feature levels (the plan keeps levels 1 and 2 as "stem" and "pool") and the five logits."""
    channels = (64, 128, 256, 512, 512, 512)
    for name, f, C in zip(("stem", "pool", "c2", "c3", "c4", "c5"), feats, channels):
        got = eng.tensor(name).permute(0, 3, 1, 2).cpu().double()
        assert got.shape == f.shape and got.shape[1] == C, name
        err = (got - f).abs().max().item()
        print(what, name, "err", err, "ref max", f.abs().max().item())
        assert err <= tol * max(1.0, f.abs().max().item()), (what, name, err)
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = logits[k].cpu().double()
        assert got.shape == ref[k].shape, k
        err = (got - ref[k]).abs().max().item()
        print(what, k, "err", err, "ref max", ref[k].abs().max().item())
        assert err <= tol * max(1.0, ref[k].abs().max().item()), (what, k, err)


@pytest.mark.parametrize("encoder,B,H,W", V.ENGINE_CASES)
def test_engine_vs_float64_cpu(lib, dev, encoder, B, H, W):
    """The plan as the model builds and tunes it, then with every wino-eligible site forced to Winograd form 9 (the fp16-piece form of
    the headline): each against the float64 module at 1e-4 max(1, |ref|) on every feature level and logit."""
    m0, hp0, x, ref, feats = _float64(lib, encoder, B, H, W)
    nconv = sum(V.CONFIGS[encoder[:5]])
    assert len(feats) == 6 and tuple(feats[5].shape[2:]) == (H // 32, W // 32)
    m = copy.deepcopy(m0)
    m.HPARAM = copy.copy(hp0)
    m = m.to(dev)
    xd = x.to(dev)
    with torch.no_grad():
        out = m(xd)
    assert m._engines, "the native engine did not run"
    eng = next(iter(m._engines.values()))
    _check(eng, out["logits"], ref, feats, encoder + " tuned")
    plans = eng.conv_plans()
    assert len(plans) == nconv - 1 + 44
    enc_sites = plans[:nconv - 1]
    assert all(p[4] % 72 == 0 and p[3] % 64 == 0 for p in enc_sites)                   # 3x3 over Cin % 8 == 0 to Cout % 64 == 0: wino-eligible, all
    print(encoder, "tuned plan codes of the encoder sites:", [p[2] for p in enc_sites])
    with pytest.raises(RuntimeError):
        eng.force_fold(1)
    assert eng.force_fold(0) == 0
    with pytest.raises(RuntimeError):
        eng.force_stem_pool(0)
    assert eng.flops()[0] > 0
    # every wino-eligible site — the encoder's and the seven segmentation convolutions, one grouped launch of the four decoders each — on form 9
    assert eng.force_winograd(9) == nconv - 1 + 7
    plans = eng.conv_plans()
    assert all(p[2] == -9 for p in plans[:nconv - 1]), [p[2] for p in plans[:nconv - 1]]
    assert sum(p[2] == -9 for p in plans[nconv - 1:]) == 7
    with torch.no_grad():
        out9 = m(xd)
    assert len(m._engines) == 1
    _check(eng, out9["logits"], ref, feats, encoder + " form 9")


def test_graph_replay_and_streamer_bit_for_bit(lib, dev):
    """vgg13 at (1, 64, 96): three forwards of the graph-recorded engine on a side stream and one frame through the streaming runtime
    (the same plan on a stream of its own) return the eager launches' bits."""
    from fastposecnn_amd.streaming import FrameStreamer
    m0, hp0 = V.model(lib, "vgg13")
    m = copy.deepcopy(m0)
    m.HPARAM = copy.copy(hp0)
    m = m.to(dev)
    xd = V.images(1, 64, 96).to(dev)
    with torch.no_grad():
        out = m(xd)                                   # (the null stream: plain launches)
    torch.cuda.synchronize()
    assert m._engines
    eng = next(iter(m._engines.values()))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        for i in range(3):
            again = m(xd)
            side.synchronize()
            for k in out["logits"]:
                assert torch.equal(again["logits"][k], out["logits"][k]), (i, k)
            assert torch.equal(again["categorical"]["mask"], out["categorical"]["mask"])
    assert len(m._engines) == 1 and eng.graph_recorded()
    st = FrameStreamer(m, net_streams=1)
    got = st.collect(st.submit(xd))
    assert len(m._engines) == 1
    for k in out["logits"]:
        assert torch.equal(got["logits"][k], out["logits"][k]), k
    assert torch.equal(got["categorical"]["mask"], out["categorical"]["mask"])


def test_training_step(lib, dev, monkeypatch):
    """One training step of vgg11_bn at (2, 64, 96) through the modules (the native front ends where they accept the shape, torch's
    2x2 pools): a finite loss, and every parameter with a finite gradient."""
    from fastposecnn_amd import config
    from fastposecnn_amd.lib import train_conv
    # a plan cache of this test's own: the front end keeps the form it timed fastest per convolution shape for the whole process, and
    # the decoders' shapes are every encoder's — what this test times must not decide what later tests run
    monkeypatch.setattr(train_conv, "_plan_cache", {})
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "vgg11_bn"
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    x = V.images(2, 64, 96).to(dev)
    out = model.pure_model_forward(x)
    loss = sum(v.square().mean() for v in out.values())
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert sum(n.startswith("encoder.features.") for n in names) == 8 * 4              # 8 convolutions: weight, bias and the BatchNorm's two
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert any(p.grad.abs().max().item() > 0 for n, p in model.named_parameters() if n.startswith("encoder.features.0."))
