"""The FPN p2 level folded into s2.0 (csrc/wino_h3.hip, FOLD): conv3x3(W, L c2 + b + up2(p3)) computed as conv3x3(W L, c2) +
conv3x3(W, up2(p3)) + a bias table by border class, without writing p2.  Held to the bars of every other convolution form."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEC = ("mask_decoder", "rotation_decoder", "translation_decoder", "scales_decoder")
LEVEL_3 = 3      # fpc_net_set_split_precision level of the engine's default front end


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


def _model(lib, encoder="resnet34", seed=0):
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = encoder
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
    for name, p in m.named_parameters():      # non-zero lateral biases: the border-class table is exercised
        if name.endswith("p2.skip_conv.bias"):
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return m.eval(), hp


def _seg6_ref(m, eng, d):
    """float64 conv3x3(W, L c2 + b + up2(p3)) from the engine's own c2 and p3 (NHWC -> NCHW)."""
    sd = dict(m.named_parameters())
    L = sd[f"{DEC[d]}.p2.skip_conv.weight"].detach().cpu().double()
    b = sd[f"{DEC[d]}.p2.skip_conv.bias"].detach().cpu().double()
    W = sd[f"{DEC[d]}.seg_blocks.3.block.0.block.0.weight"].detach().cpu().double()
    c2 = eng.tensor("c2").detach().cpu().double().permute(0, 3, 1, 2)
    p3 = eng.tensor(f"d{d}.p3").detach().cpu().double().permute(0, 3, 1, 2)
    p2 = F.conv2d(c2, L, b) + F.interpolate(p3, scale_factor=2, mode="nearest")
    return F.conv2d(p2, W, padding=1)


def _engine(m, B, H, W, dev):
    x = torch.zeros((B, 3, H, W), device=dev)
    with torch.no_grad():
        m(x)
    return m._engines[(B, H, W, x.device)]


def _check_seg6(m, eng, frames, bar=2e-5):
    for d in range(4):
        ref = _seg6_ref(m, eng, d)[frames]
        got = eng.tensor(f"d{d}.seg6").detach().cpu().double().permute(0, 3, 1, 2)[frames]
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        assert err <= bar, (d, err)


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (2, 96, 64), (1, 480, 640)])
def test_fold_seg6_against_float64(lib, dev, B, H, W):
    """s2.0's pre-GroupNorm output with p2 folded in against float64 of the same c2 / p3: 2e-5 of the tensor's scale, the bar of
    every convolution site.  96 x 64: p2 24 x 16, p3 12 x 8, a tile patch row that is cut at the bottom border."""
    from fastposecnn_amd import synth
    m, _ = _model(lib)
    m = m.to(dev)
    eng = _engine(m, B, H, W, dev)
    eng.force_fold(1)
    x = torch.stack([synth.make_image(i, H, W) for i in range(B)]).to(dev)
    with torch.no_grad():
        m(x)
    assert eng.conv_plans() and any(p[2] == 5000 for p in eng.conv_plans())
    _check_seg6(m, eng, list(range(B)))
    with pytest.raises(Exception):
        eng.tensor("d0.p2")          # never written while folded


def test_fold_logits_within_1e4_of_float64(lib, dev):
    """The whole network with the fold forced: the logits against the float64 CPU module path at 1e-4 of each tensor's scale."""
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
    with torch.no_grad():
        out = m(x.to(dev))
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = out["logits"][k].cpu().double()
        err = (got - ref[k]).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref[k].abs().max().item()), (k, err)


def test_fold_plan_rules(lib, dev):
    """force_winograd(8) unfolds, force_winograd(9) keeps the fold; an engine without the fp16 forms never picks it; copied plans
    carry it."""
    m, _ = _model(lib)
    m = m.to(dev)
    eng = _engine(m, 2, 64, 96, dev)
    assert eng.force_fold(1) in (0, 1)
    eng.force_winograd(9)
    assert any(p[2] == 5000 for p in eng.conv_plans())
    eng.force_winograd(8)
    assert not any(p[2] == 5000 for p in eng.conv_plans())
    eng.force_fold(1)
    e1 = _engine(m, 1, 64, 96, dev)
    e1.copy_plans_from(eng)
    assert e1.conv_plans() == eng.conv_plans()
    m2, hp2 = _model(lib)
    hp2.ENGINE_SPLIT_F16 = False
    m2 = m2.to(dev)
    e2 = _engine(m2, 2, 64, 96, dev)
    assert not any(p[2] == 5000 for p in e2.conv_plans())


def test_fold_graph_replay_is_bit_identical(lib, dev):
    """With the fold, replayed graphs give the plain launches' logits bit for bit, frame after frame."""
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m, _ = _model(lib)
    m = m.to(dev)
    xs = [torch.stack([synth.make_image(i + j, 64, 96) for j in range(2)]).to(dev) for i in range(3)]
    side = torch.cuda.Stream(device=dev)
    runs = []
    for graph in (False, True):
        with torch.no_grad(), torch.cuda.stream(side):
            eng = NetEngine(m, 2, 64, 96, dev, autotune=False, graph=graph, split_precision=LEVEL_3)
            assert eng.force_fold(1) == 1
            outs = []
            for x in xs + xs:
                logits, _ = eng.forward(x)
                outs.append({k: v.clone() for k, v in logits.items()})
        side.synchronize()
        runs.append(outs)
    for a, b in zip(*runs):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_headline_batch32_picks_the_fold_and_meets_the_bar(lib, dev):
    """ResNet34, B = 32, 640 x 480 (bench.py's headline): the autotuner keeps the fold (it beats the p2 lateral + s2.0), and s2.0's
    output of frames 0 and 31 meets 2e-5 of float64."""
    from fastposecnn_amd import synth
    m, _ = _model(lib)
    m = m.to(dev)
    x = torch.stack([synth.make_image(i) for i in range(32)]).to(dev)
    with torch.no_grad():
        m(x)
    eng = m._engines[(32, 480, 640, x.device)]
    plans = eng.conv_plans()
    print("batch-32 plans:", plans)
    assert any(p[2] == 5000 for p in plans), "the autotuner did not keep the fold at the headline configuration"
    _check_seg6(m, eng, [0, 31])
