"""The ResNeXt-50 (32x4d) encoder on the MI355X: the engine's plan (grouped conv2 sites on k_conv3x3_grouped) against the float64
CPU module path at the network bar 1e-4 max(1, scale), at split level 0 and the default, with and without graph replay, after
autotuning, at full size; the whole PoseRegressor forward; one training-mode forward + backward."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

ENC = "resnext50_32x4d"
FPC_PLAN_GROUPED = 8000


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


def _model(lib, seed=0):
    """Random init with perturbed BatchNorm / GroupNorm statistics, as the ResNet-50 tests."""
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = ENC
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


_REFS = {}


def _float64(lib, B, H, W):
    """(model on the CPU, hp, x, float64 logits, float64 encoder features) of a frame size, computed once and left unchanged."""
    key = (B, H, W)
    if key not in _REFS:
        from fastposecnn_amd import synth
        m, hp = _model(lib)
        x = torch.stack([synth.make_image(i, H, W) for i in range(B)])
        ref_m = copy.deepcopy(m).double()
        ref_m.HPARAM = copy.copy(hp)
        ref_m.HPARAM.USE_NATIVE_ENGINE = False
        with torch.no_grad():
            _REFS[key] = (m, hp, x, ref_m.pure_model_forward(x.double()), ref_m.encoder(x.double()))
    return _REFS[key]


def _check(eng, logits, ref, feats, tol=1e-4):
    for name, f in zip(("c2", "c3", "c4", "c5"), feats[2:]):
        got = eng.tensor(name).permute(0, 3, 1, 2).cpu().double()
        assert got.shape == f.shape, name
        err = (got - f).abs().max().item()
        assert err <= tol * max(1.0, f.abs().max().item()), (name, err)
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = logits[k].cpu().double()
        assert got.shape == ref[k].shape, k
        err = (got - ref[k]).abs().max().item()
        assert err <= tol * max(1.0, ref[k].abs().max().item()), (k, err)


def _grouped_sites(eng):
    return [p for p in eng.conv_plans() if FPC_PLAN_GROUPED <= p[2] < FPC_PLAN_GROUPED + 1000]


@pytest.mark.parametrize("split", ["default", "f32"])
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 96, 128)])
def test_engine_vs_float64_cpu(lib, dev, B, H, W, split):
    """Through the model's own forward (the engine autotunes on its first frame): the bar holds after the autotuning pass."""
    m, hp, x, ref, feats = _float64(lib, B, H, W)
    m = copy.deepcopy(m)
    m.HPARAM = copy.copy(hp)
    if split == "f32":
        m.HPARAM.ENGINE_SPLIT_PRECISION = False
    m = m.to(dev)
    with torch.no_grad():
        out = m(x.to(dev))
    assert m._engines, "the native engine did not run"
    eng = next(iter(m._engines.values()))
    _check(eng, out["logits"], ref, feats)
    assert len(_grouped_sites(eng)) == 16
    if split == "f32":
        assert not any(4000 <= p[2] < FPC_PLAN_GROUPED for p in eng.conv_plans())


def test_heuristic_and_tuned_plans_graph_on_and_off(lib, dev):
    """The heuristic plan and the autotuned one both hold the bar; graph replay of a plan returns the plain launches' bits; plans
    copied to another batch size keep the grouped sites."""
    from fastposecnn_amd.engine import NetEngine
    m, hp, x, ref, feats = _float64(lib, 2, 64, 96)
    m = copy.deepcopy(m).to(dev)
    xd = x.to(dev)
    for tune in (False, True):
        eng = NetEngine(m, 2, 64, 96, dev, autotune=tune, split_precision=3)
        logits, cat = eng.forward(xd)
        torch.cuda.synchronize()
        _check(eng, logits, ref, feats)
        assert len(_grouped_sites(eng)) == 16
        side = torch.cuda.Stream(device=dev)       # (a graph is captured on a stream of its own, never on the null stream)
        with torch.cuda.stream(side):
            engg = NetEngine(m, 2, 64, 96, dev, autotune=False, split_precision=3, graph=True)
            engg.copy_plans_from(eng)
            assert engg.conv_plans() == eng.conv_plans()
            for i in range(3):
                lg, cg = engg.forward(xd)
                side.synchronize()
                for k in logits:
                    assert torch.equal(lg[k], logits[k]), (tune, i, k)
                assert torch.equal(cg["mask"], cat["mask"])
        assert engg.graph_recorded()
    one = NetEngine(m, 1, 64, 96, dev, autotune=False, split_precision=3)
    one.copy_plans_from(eng)
    assert len(_grouped_sites(one)) == 16
    l1, _ = one.forward(xd[:1])
    torch.cuda.synchronize()
    for k in logits:
        assert (l1[k].cpu().double() - ref[k][:1]).abs().max().item() <= 1e-4 * max(1.0, ref[k].abs().max().item()), k


def test_fullsize_vs_float64(lib, dev):
    from fastposecnn_amd.engine import NetEngine
    m, hp, x, ref, feats = _float64(lib, 1, 480, 640)
    m = copy.deepcopy(m).to(dev)
    eng = NetEngine(m, 1, 480, 640, dev, autotune=True, split_precision=3)
    logits, _ = eng.forward(x.to(dev))
    torch.cuda.synchronize()
    _check(eng, logits, ref, feats)
    print("resnext50 B=1 plans:", eng.conv_plans())


def test_pipeline_and_streamer(lib, dev):
    """PoseRegressor.forward end to end on a ResNeXt model returns the reference's key set, and the streaming runtime agrees."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.streaming import FrameStreamer
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.HV_NUM_OF_HYPOTHESES = 128
    hp.ENCODER = ENC
    torch.manual_seed(0)
    m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).to(dev).eval()
    H, W = 96, 128
    x0 = synth.make_image(0, H, W)[None].to(dev)
    with torch.no_grad():
        full = m(x0)
    assert set(full) == {"logits", "categorical", "aggregated"}
    assert full["categorical"]["mask"].dtype == torch.int64 and tuple(full["categorical"]["mask"].shape) == (1, H, W)
    cat0, _ = synth.make_vote_frame(0, K=3, H=H, W=W, rmin=8, rmax=20)
    cat0 = {k: v.to(dev) for k, v in cat0.items()}
    with torch.no_grad():
        logits = m.pure_model_forward(x0)
        torch.manual_seed(100)
        agg = m.agg_hough_and_generate_RT(cat0)
    st = FrameStreamer(m)
    torch.manual_seed(99)
    st.prepare(x0, categorical_override=cat0)
    torch.manual_seed(100)
    out = st.collect(st.submit(x0, categorical_override=cat0))
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        a, b = out["logits"][k], logits[k]
        assert (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item()), k
    assert set(out["aggregated"]) == set(agg)
    for k, v in agg.items():
        assert torch.equal(out["aggregated"][k], v), k


def test_grouped_conv_module_leaves_the_counters_alone(lib, dev):
    """Training mode on the GPU: the grouped Conv2d is torch's grouped convolution on the channel-last tensor, forward and
    backward, and is counted neither as native nor as aten."""
    from fastposecnn_amd.lib import backbone as bb, train_conv
    torch.manual_seed(2)
    c = bb.Conv2d(128, 128, 3, 2, 1, groups=32, bias=False).to(dev).train()
    x = torch.randn(2, 128, 9, 12, device=dev, requires_grad=True)
    before = dict(train_conv.counters)
    y = c(x)
    y.square().sum().backward()
    torch.cuda.synchronize()
    assert dict(train_conv.counters) == before
    assert y.is_contiguous(memory_format=torch.channels_last)
    xr = x.detach().double().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, c.weight.detach().double(), None, 2, 1, 1, 32)
    yr.square().sum().backward()
    assert (y.double() - yr).abs().max().item() <= 2e-5 * max(1.0, yr.abs().max().item())
    assert (x.grad.double() - xr.grad).abs().max().item() <= 1e-4 * max(1.0, xr.grad.abs().max().item())


def test_training_step_native_vs_torch(lib, dev, monkeypatch):
    """Forward + backward of the model in training mode at B = 1, 64 x 96: native convolutions (the grouped ones on torch) against
    the same model on torch's f32 kernels, each against float64 — the bars of test_resnet50_training_step_native_vs_torch."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = ENC
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
        for name, child in list(mod.named_children()):
            if isinstance(child, torch.nn.ReLU):
                setattr(mod, name, torch.nn.Softplus())
    dense = sum(1 for mod in model.modules() if isinstance(mod, torch.nn.Conv2d) and mod.groups == 1)
    grouped = sum(1 for mod in model.modules() if isinstance(mod, torch.nn.Conv2d) and mod.groups > 1)
    assert grouped == 16
    x = synth.make_image(0, 64, 96)[None].to(dev)
    res = {}
    for tag in ("native", "torch32", "torch64"):
        monkeypatch.setattr(train_conv, "ENABLED", tag == "native")
        if tag == "torch64":
            model = model.double()
            x = x.double()
        model.zero_grad(set_to_none=True)
        before = dict(train_conv.counters)
        out = model.pure_model_forward(x)
        loss = sum(v.square().mean() for v in out.values())
        loss.backward()
        torch.cuda.synchronize()
        used = {k: train_conv.counters[k] - before[k] for k in before}
        res[tag] = (loss.item(), {k: v.detach().double() for k, v in out.items()},
                    {n: p.grad.detach().double() for n, p in model.named_parameters() if p.grad is not None}, used)
    ln, on, gn, used = res["native"]
    lt, ot, gt, unused = res["torch32"]
    lr, orf, gr, _ = res["torch64"]
    # the dense convolutions but the stem run native (ResNeXt-50: 36 encoder 1x1, 44 decoder convolutions, 4 heads); the 16 grouped
    # ones appear in no counter, so no count can exceed the dense sites
    assert dense - 1 == 84 and 60 <= used["fwd_native"] <= dense - 1, (used, dense)
    assert used["wgrad_native"] + used["wgrad_aten"] <= dense - 1 and used["dgrad_native"] + used["dgrad_aten"] <= dense - 1, used
    assert unused["fwd_native"] == 0
    assert abs(ln - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in orf:
        assert (on[k] - orf[k]).abs().max().item() <= 1e-4 * max(1.0, orf[k].abs().max().item()), k
    assert set(gn) == set(gr)
    err_n = err_t = 0.0
    for n in gr:
        scale = max(gr[n].abs().max().item(), 1e-12)
        err_n = max(err_n, (gn[n] - gr[n]).abs().max().item() / scale)
        err_t = max(err_t, (gt[n] - gr[n]).abs().max().item() / scale)
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)
