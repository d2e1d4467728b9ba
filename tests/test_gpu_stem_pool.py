"""k_stem_pool_h3 (fpc_conv2d's request 3100, plan code 3100 at the stem site): the 7x7 / stride-2 stem, folded BatchNorm, ReLU and the
3x3 / stride-2 / pad-1 max-pool as one launch on three fp16 piece products.  A wave walks down a strip of 64 conv columns over a band
of 10 pool rows; the conv column left of a strip is recomputed (one 32-pixel tile per task).  Held to the 2e-5 bar of every other
convolution form against float64 max_pool2d(relu(bn(conv2d))), on shapes whose outputs contain band and strip boundaries, with
inputs that make a missing halo column or row visible, over the operand ranges of the fp16-piece forms, and in the whole network."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

STEM_POOL = 3100     # fpc_conv2d request: `out` is the pooled tensor [B][Ho / 2][Wo / 2][64]
BAND = 10            # pool rows per wave task (net_kernels.hpp: kStemPoolBand); a strip is 32 pool columns


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


def _stem_pool(dev, x, w, scale=None, shift=None, frames=None):
    """x [B,3,H,W], w [64,3,7,7] -> pooled [B',64,Hp,Wp] on the CPU (B' = the frames asked for)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, _, Hi, Wi = x.shape
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    x4 = torch.cat([x, torch.zeros(B, 1, Hi, Wi)], 1).permute(0, 2, 3, 1).contiguous().to(dev)      # NHWC4, 4th channel 0
    w4 = torch.cat([w, torch.zeros(64, 1, 7, 7)], 1).contiguous().to(dev)
    sb, sh, sw, sc = x4.stride()
    out = torch.full((B, Ho // 2, Wo // 2, 64), float("nan"), device=dev)
    ws = torch.empty(L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, 4, 64, 7, 7, 0, 0, STEM_POOL), dtype=torch.uint8, device=dev)
    t = lambda a: None if a is None else a.contiguous().to(dev)
    scale_d, shift_d = t(scale), t(shift)
    nat.check(L.fpc_conv2d(x4.data_ptr(), sb, sh, sw, sc, w4.data_ptr(), nat.ptr(scale_d), nat.ptr(shift_d), None, None,
                           out.data_ptr(), None, B, Hi, Wi, 4, 64, 7, 7, 2, 3, 1, 0, 0, STEM_POOL, ws.data_ptr(), ws.numel(),
                           nat.stream()), "conv2d")
    torch.cuda.synchronize()
    if frames is not None:
        out = out[list(frames)]
    return out.permute(0, 3, 1, 2).cpu()


def _ref(x, w, scale=None, shift=None):
    y = F.conv2d(x.double(), w.double(), stride=2, padding=3)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    return F.max_pool2d(y.relu(), 3, 2, 1)


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


def _operands(B, Hi, Wi, g, bn, xs=1.0, wsc=None):
    x = torch.randn(B, 3, Hi, Wi, generator=g) * xs      # a normalised image: both signs
    w = torch.randn(64, 3, 7, 7, generator=g) * (wsc if wsc is not None else (2.0 / 147) ** 0.5)
    kw = {}
    if bn:
        kw["scale"] = torch.rand(64, generator=g) + 0.5
        kw["shift"] = torch.randn(64, generator=g) * 0.1
    return x, w, kw


# B, Hi, Wi, frames compared (None: all).  Pool rows per frame Hi / 4, strips Wi / 128; 2 048 waves in the launch.
SHAPES = [
    (2, 96, 128, None),       # 24 pool rows (bands 10 + 10 + 4), one strip: every row border class, short last band
    (3, 40, 256, None),       # 10 pool rows, two strips: every column border class and a strip boundary
    (1, 480, 640, None),      # the headline frame: 12 bands x 5 strips = 60 tasks, fewer than waves
    (32, 480, 640, (0, 31)),  # the headline batch: 1 920 tasks; first and last frame
    (90, 480, 256, (0, 44, 89)),   # 12 bands x 2 strips x 90 = 2 160 tasks, more than waves: a second round of the walk
    (1, 88, 384, None),       # 22 pool rows (10 + 10 + 2), three strips
]


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("B,Hi,Wi,frames", SHAPES)
def test_stem_pool_against_float64(lib, dev, B, Hi, Wi, frames, bn):
    g = torch.Generator().manual_seed(B * 1000 + Hi + Wi)
    x, w, kw = _operands(B, Hi, Wi, g, bn)
    got = _stem_pool(dev, x, w, frames=frames, **kw)
    sel = x if frames is None else x[list(frames)]
    ref = _ref(sel, w, **kw)
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()          # (the output starts as NaN: every element was written)
    assert _rel(got, ref) <= 2e-5
    Hp, Wp = ref.shape[2:]
    if (Hi, Wi) != (96, 128) and (Hi, Wi) != (40, 256):
        assert Hp > BAND and Wp > 32          # a band boundary and a strip boundary lie inside the checked output
    # ... and hold the boundary rows / columns to the bar on their own scale
    for r in (BAND - 1, BAND):
        if r < Hp:
            assert _rel(got[:, :, r], ref[:, :, r]) <= 2e-5
    for c in (31, 32):
        if c < Wp:
            assert _rel(got[:, :, :, c], ref[:, :, :, c]) <= 2e-5


def test_stem_pool_halo_column(lib, dev):
    """One bright image column whose conv response peaks in the LAST conv column of strip 0 (conv column 63 = image column 126): pool
    column 32, the first of strip 1, takes its maximum from that conv column alone (conv columns 64 and 65 respond far less).  A
    missing halo leaves it near zero."""
    Hi, Wi = 96, 384
    x = torch.zeros(1, 3, Hi, Wi)
    x[:, :, :, 126] = 2.0
    g = torch.Generator().manual_seed(21)
    w = torch.randn(64, 3, 7, 7, generator=g).abs() * 0.01
    w[:, :, :, 3] = 1.0 + torch.rand(64, 3, 7, generator=g)      # the centre tap dominates: the response peaks where the column is centred
    got = _stem_pool(dev, x, w)
    ref = _ref(x, w)
    conv = F.conv2d(x.double(), w.double(), stride=2, padding=3)
    assert (conv[..., 63] > 20 * conv[..., 64].abs()).all() and (conv[..., 63] > 20 * conv[..., 65].abs()).all()
    col = ref[:, :, :, 32]
    assert (got[:, :, :, 32].double() - col).abs().max().item() <= 2e-5 * col.abs().max().item()
    assert col.min().item() > 1.0
    assert _rel(got, ref) <= 2e-5


def test_stem_pool_halo_row(lib, dev):
    """The same for the last conv row of a band: a bright image row centred on conv row 19 (image row 38), the last row of band 0;
    pool row 10, the first of band 1, takes its maximum from it."""
    Hi, Wi = 96, 256
    x = torch.zeros(1, 3, Hi, Wi)
    x[:, :, 38, :] = 2.0
    g = torch.Generator().manual_seed(22)
    w = torch.randn(64, 3, 7, 7, generator=g).abs() * 0.01
    w[:, :, 3, :] = 1.0 + torch.rand(64, 3, 7, generator=g)
    got = _stem_pool(dev, x, w)
    ref = _ref(x, w)
    conv = F.conv2d(x.double(), w.double(), stride=2, padding=3)
    assert (conv[:, :, 19] > 20 * conv[:, :, 20].abs()).all() and (conv[:, :, 19] > 20 * conv[:, :, 21].abs()).all()
    row = ref[:, :, 10]
    assert (got[:, :, 10].double() - row).abs().max().item() <= 2e-5 * row.abs().max().item()
    assert row.min().item() > 1.0
    assert _rel(got, ref) <= 2e-5


@pytest.mark.parametrize("xs", [1e-2, 1.0, 1e3])
@pytest.mark.parametrize("wsc", [1e-4, 1e-2, 1e2])
def test_stem_pool_operand_ranges(lib, dev, xs, wsc):
    g = torch.Generator().manual_seed(11)
    x, w, kw = _operands(2, 88, 256, g, True, xs=xs, wsc=wsc)
    kw["shift"] = kw["shift"] * xs * wsc
    got = _stem_pool(dev, x, w, **kw)
    assert _rel(got, _ref(x, w, **kw)) <= 2e-5


def test_stem_pool_outlier_stays_finite(lib, dev):
    g = torch.Generator().manual_seed(5)
    x, w, kw = _operands(1, 96, 128, g, True)
    x[0, 1, 37, 61] = 1e6
    got = _stem_pool(dev, x, w, **kw)
    assert torch.isfinite(got).all()


def test_stem_pool_refuses_ineligible(lib, dev):
    """No ReLU (the pool's zero padding rests on it), an odd conv height, a conv width that is no multiple of 64."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    for Hi, Wi, relu in ((96, 128, 0), (98, 128, 1), (96, 192, 1)):
        Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
        x4 = torch.zeros(1, Hi, Wi, 4, device=dev)
        w4 = torch.zeros(64, 4, 7, 7, device=dev)
        out = torch.zeros(1, max(Ho // 2, 1), max(Wo // 2, 1), 64, device=dev)
        ws = torch.empty(L.fpc_conv2d_workspace_bytes(1, Ho, Wo, 4, 64, 7, 7), dtype=torch.uint8, device=dev)
        sb, sh, sw, sc = x4.stride()
        rc = L.fpc_conv2d(x4.data_ptr(), sb, sh, sw, sc, w4.data_ptr(), None, None, None, None, out.data_ptr(), None, 1, Hi, Wi, 4, 64,
                          7, 7, 2, 3, relu, 0, 0, STEM_POOL, ws.data_ptr(), ws.numel(), nat.stream())
        assert rc == -1, (Hi, Wi, relu, rc)      # FPC_EINVAL


def test_stem_pool_repeat_bit_identical(lib, dev):
    g = torch.Generator().manual_seed(3)
    x, w, kw = _operands(2, 480, 640, g, True)
    assert torch.equal(_stem_pool(dev, x, w, **kw), _stem_pool(dev, x, w, **kw))


# ---- the network with the stem site on the fused form

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


def test_network_on_stem_pool_within_1e4_of_float64(lib, dev):
    """ResNet34 with the stem site forced onto the fused launch, the p2 fold and the nine direct h3 sites kept: logits and c2 within
    1e-4 of the float64 module path, "pool" within 2e-5, "stem" refused; two forwards bit-identical."""
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m, hp = _model(lib)
    x = torch.stack([synth.make_image(i, 96, 128) for i in range(2)])
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp); ref_m.HPARAM.USE_NATIVE_ENGINE = False
    with torch.no_grad():
        ref = ref_m.pure_model_forward(x.double())
    m = m.to(dev)
    eng = NetEngine(m, 2, 96, 128, dev, autotune=False, split_precision=3)
    eng.force_fold(1)
    assert eng.force_direct_h3(1) == 9
    assert eng.force_stem_pool(1) == 1 and eng.force_stem_pool(1) == 0
    plans = eng.conv_plans()
    assert sum(1 for p in plans if p[2] == 3100) == 1
    assert sum(1 for p in plans if 6000 <= p[2] < 6200 or 7000 <= p[2] < 8000) == 9 and any(p[2] == 5000 for p in plans)
    with torch.no_grad():
        logits, _ = eng.forward(x.to(dev))
        logits = {k: v.clone() for k, v in logits.items()}
        logits2, _ = eng.forward(x.to(dev))
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = logits[k].cpu().double()
        err = (got - ref[k]).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref[k].abs().max().item()), (k, err)
        assert torch.equal(logits[k], logits2[k]), k
    with pytest.raises(Exception):
        eng.tensor("stem")
    # float64 encoder front end from the module's own layers
    e64 = _encoder(ref_m)
    with torch.no_grad():
        pool64 = e64.maxpool(e64.relu(e64.bn1(e64.conv1(x.double()))))
        c2_64 = e64.layer1(pool64)
    pool = eng.tensor("pool").permute(0, 3, 1, 2).cpu().double()
    assert (pool - pool64).abs().max().item() <= 2e-5 * pool64.abs().max().item()
    c2 = eng.tensor("c2").permute(0, 3, 1, 2).cpu().double()
    assert (c2 - c2_64).abs().max().item() <= 1e-4 * max(1.0, c2_64.abs().max().item())
    assert eng.force_stem_pool(0) == 1
    assert eng.tensor("stem").shape[-1] == 64


def _encoder(model):
    for mod in model.modules():
        if all(hasattr(mod, a) for a in ("conv1", "bn1", "relu", "maxpool", "layer1", "layer4")):
            return mod
    raise AssertionError("no ResNet encoder in the model")


def test_stem_pool_needs_split_level_3(lib, dev):
    from fastposecnn_amd.engine import NetEngine
    m, _ = _model(lib)
    m = m.to(dev)
    eng = NetEngine(m, 1, 64, 128, dev, autotune=False, split_precision=1)
    with pytest.raises(Exception):
        eng.force_stem_pool(1)


def test_network_stem_pool_batch32_graph_replay_bit_equal(lib, dev):
    """ResNet34 at batch 32, 640 x 480 with the stem site on the fused launch: replayed graphs give the plain launches' logits bit
    for bit, and repeats are bit-identical."""
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
            assert eng.force_stem_pool(1) == 1
            outs = []
            for x in xs + xs:
                logits, _ = eng.forward(x)
                outs.append({k: v.clone() for k, v in logits.items()})
        side.synchronize()
        assert eng._lib.fpc_net_graph_recorded(eng._h) == (1 if graph else 0)
        assert any(p[2] == 3100 for p in eng.conv_plans())
        runs.append(outs)
        del eng
    for a, b in zip(*runs):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[0][2][k]), k      # the same frames again: bit-identical
