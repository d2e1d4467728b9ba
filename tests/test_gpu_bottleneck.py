"""The Bottleneck encoders on the MI355X: k_conv1x1 (csrc/pointwise.hip) against float64 through fpc_conv2d, and the engine's
ResNet-50 / 101 plans against the float64 CPU module path, the torch-module path, the streaming runtime and the training step."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


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


def _conv1x1(dev, x, w, stride, nsplit, scale=None, shift=None, res=None, up=None, relu=False):
    """fpc_conv2d on NHWC input, 1x1 / pad 0; returns (rc, out NCHW on the CPU)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, Cin, Hi, Wi = x.shape
    Cout = w.shape[0]
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    xin = x.permute(0, 2, 3, 1).contiguous().to(dev)
    sb, sh, sw, sc = xin.stride()
    wd = w.contiguous().to(dev)
    out = torch.full((B, Ho, Wo, Cout), float("nan"), device=dev)
    t = lambda a: None if a is None else a.contiguous().to(dev)
    nhwc = lambda a: None if a is None else a.permute(0, 2, 3, 1).contiguous().to(dev)
    scale_d, shift_d, res_d, up_d = t(scale), t(shift), nhwc(res), nhwc(up)
    ws = torch.empty(L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, Cin, Cout, 1, 1, 0, 0, nsplit), dtype=torch.uint8, device=dev)
    rc = L.fpc_conv2d(xin.data_ptr(), sb, sh, sw, sc, wd.data_ptr(), nat.ptr(scale_d), nat.ptr(shift_d), nat.ptr(res_d),
                      nat.ptr(up_d), out.data_ptr(), None, B, Hi, Wi, Cin, Cout, 1, 1, stride, 0, int(relu), 0, 0, nsplit,
                      ws.data_ptr(), ws.numel(), nat.stream())
    torch.cuda.synchronize()
    return rc, out.permute(0, 3, 1, 2).cpu()


def _ref(x, w, stride, scale=None, shift=None, res=None, up=None, relu=False):
    y = F.conv2d(x.double(), w.double(), stride=stride)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if up is not None:
        y = y + F.interpolate(up.double(), scale_factor=2, mode="nearest")
    return y.relu() if relu else y


# every 1x1 shape of ResNet-50 (Cin, Cout, stride, epilogue) on small maps; the laterals with their top-down addend
R50_1X1 = [
    (64, 64, 1, "bn_relu"), (256, 64, 1, "bn_relu"), (64, 256, 1, "bn_res_relu"), (64, 256, 1, "bn"),           # layer1
    (256, 128, 1, "bn_relu"), (512, 128, 1, "bn_relu"), (128, 512, 1, "bn_res_relu"), (256, 512, 2, "bn"),      # layer2
    (512, 256, 1, "bn_relu"), (1024, 256, 1, "bn_relu"), (256, 1024, 1, "bn_res_relu"), (512, 1024, 2, "bn"),   # layer3
    (1024, 512, 1, "bn_relu"), (2048, 512, 1, "bn_relu"), (512, 2048, 1, "bn_res_relu"), (1024, 2048, 2, "bn"), # layer4
    (2048, 256, 1, "bias"), (1024, 256, 1, "bias_up"), (512, 256, 1, "bias_up"), (256, 256, 1, "bias_up"),     # laterals
]
CASES = [(B, Hi, Wi, *shape, v) for shape in R50_1X1 for (B, Hi, Wi) in ((1, 10, 14), (3, 6, 10)) for v in (0, 1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}-{c[1]}x{c[2]}-{c[3]}-{c[4]}-s{c[5]}-{c[6]}-v{c[7]}")
def test_conv1x1_vs_float64(lib, dev, case):
    """B = 1 at 10 x 14 (140 pixels) and B = 3 at 6 x 10 (180): M is never a multiple of the 64 / 128-pixel tile, and tiles
    cross image boundaries.  Bar and weight scale of test_gpu_net.py's CONV_CASES.  Two calls are bit-identical."""
    B, Hi, Wi, Cin, Cout, stride, extra, variant = case
    g = torch.Generator().manual_seed(CASES.index(case))
    x = torch.randn((B, Cin, Hi, Wi), generator=g)
    w = torch.randn((Cout, Cin, 1, 1), generator=g) / Cin ** 0.5
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    kw = {}
    if "bn" in extra:
        kw["scale"] = torch.rand(Cout, generator=g) + 0.5
        kw["shift"] = torch.randn(Cout, generator=g)
    if "bias" in extra:
        kw["shift"] = torch.randn(Cout, generator=g)
    if "res" in extra:
        kw["res"] = torch.randn((B, Cout, Ho, Wo), generator=g)
    if "up" in extra:
        kw["up"] = torch.randn((B, Cout, Ho // 2, Wo // 2), generator=g)
    kw["relu"] = "relu" in extra
    rc, out = _conv1x1(dev, x, w, stride, 4000 + variant, **kw)
    assert rc == 0
    ref = _ref(x, w, stride, **kw)
    assert not torch.isnan(out).any(), "unwritten outputs"
    err = (out.double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err
    rc2, out2 = _conv1x1(dev, x, w, stride, 4000 + variant, **kw)
    assert rc2 == 0 and torch.equal(out, out2)


def test_conv1x1_refuses_what_it_does_not_take(lib, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, 96, 6, 8), generator=g)                           # Cin not a multiple of 64
    assert _conv1x1(dev, x, torch.randn((64, 96, 1, 1), generator=g), 1, 4000)[0] == -1
    x = torch.randn((1, 64, 6, 8), generator=g)
    assert _conv1x1(dev, x, torch.randn((96, 64, 1, 1), generator=g), 1, 4000)[0] == -1     # Cout not a multiple of 64
    assert _conv1x1(dev, x, torch.randn((64, 64, 1, 1), generator=g), 1, 4002)[0] == -1     # no such variant


def _model(lib, encoder, seed=0):
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
    return m.eval(), hp


def _float64(m, hp, x):
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp)
    ref_m.HPARAM.USE_NATIVE_ENGINE = False
    with torch.no_grad():
        return ref_m.pure_model_forward(x.double()), ref_m.encoder(x.double())


def _check(eng, out, ref, feats, tol=1e-4):
    for name, f in zip(("c2", "c3", "c4", "c5"), feats[2:]):
        got = eng.tensor(name).permute(0, 3, 1, 2).cpu().double()
        assert got.shape == f.shape, name
        err = (got - f).abs().max().item()
        assert err <= tol * max(1.0, f.abs().max().item()), (name, err)
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = out["logits"][k].cpu().double()
        assert got.shape == ref[k].shape, k
        err = (got - ref[k]).abs().max().item()
        assert err <= tol * max(1.0, ref[k].abs().max().item()), (k, err)


@pytest.mark.parametrize("split", ["default", "no-f16", "f32"])
@pytest.mark.parametrize("encoder,B,H,W", [("resnet50", 2, 64, 96), ("resnet101", 1, 96, 64)])
def test_engine_vs_float64_cpu(lib, dev, encoder, B, H, W, split):
    from fastposecnn_amd import synth
    m, hp = _model(lib, encoder)
    if split == "no-f16":
        hp.ENGINE_SPLIT_F16 = False
    if split == "f32":
        hp.ENGINE_SPLIT_PRECISION = False
    x = torch.stack([synth.make_image(i, H, W) for i in range(B)])
    ref, feats = _float64(m, hp, x)
    m = m.to(dev)
    with torch.no_grad():
        out = m(x.to(dev))
    assert m._engines, "the native engine did not run"
    eng = next(iter(m._engines.values()))
    _check(eng, out, ref, feats)
    plans = eng.conv_plans()
    if split == "f32":
        assert not any(p[2] >= 4000 for p in plans)                       # level 0: k_conv_igemm's f32 form only


def _count_1x1_sites(m):
    """The model's 1x1 convolutions as plan sites: every encoder 1x1, and the laterals once per level (the four decoders'
    laterals of a level are one grouped launch sharing its input)."""
    enc = sum(1 for mod in m.encoder.modules() if isinstance(mod, torch.nn.Conv2d) and mod.kernel_size == (1, 1))
    lat = sum(1 for mod in m.mask_decoder.modules() if isinstance(mod, torch.nn.Conv2d) and mod.kernel_size == (1, 1))
    return enc + lat


def test_forced_pointwise_fullsize_vs_float64(lib, dev):
    """ResNet-50 at 640 x 480, B = 1, every 1x1 site on k_conv1x1; graph replay of the forced plan is bit-identical."""
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m, hp = _model(lib, "resnet50")
    x = synth.make_image(0)[None]
    ref, feats = _float64(m, hp, x)
    m = m.to(dev)
    eng = NetEngine(m, 1, 480, 640, dev, autotune=True, split_precision=3)
    n = _count_1x1_sites(m)
    assert n == 36 + 4
    already = sum(1 for p in eng.conv_plans() if 4000 <= p[2] < 5000)         # sites the autotuner put there itself
    assert eng.force_pointwise(1) == n - already
    assert sum(1 for p in eng.conv_plans() if 4000 <= p[2] < 5000) == n
    xd = x.to(dev)
    logits, _ = eng.forward(xd)
    torch.cuda.synchronize()
    _check(eng, {"logits": logits}, ref, feats)
    eng2 = NetEngine(m, 1, 480, 640, dev, autotune=True, split_precision=3, graph=True)
    eng2.force_pointwise(1)
    outs = []
    for _ in range(3):
        lg, cat = eng2.forward(xd)
        torch.cuda.synchronize()
        outs.append((lg, cat))
    for k in logits:
        assert torch.equal(outs[1][0][k], outs[2][0][k]), k
        assert torch.equal(outs[0][0][k], outs[2][0][k]), k
    assert torch.equal(outs[1][1]["mask"], outs[2][1]["mask"])
    assert eng.force_pointwise(0) == n and not any(4000 <= p[2] < 5000 for p in eng.conv_plans())


def test_resnet50_b32_fullsize_vs_torch_modules(lib, dev):
    import gpu_tensor_funcs as gtf
    from fastposecnn_amd import synth
    m, hp = _model(lib, "resnet50")
    m = m.to(dev)
    B = 32
    x = torch.stack([synth.make_image(i) for i in range(B)]).to(dev)
    with torch.no_grad():
        out = m(x)
    assert m._engines
    eng = next(iter(m._engines.values()))
    m.HPARAM.USE_NATIVE_ENGINE = False
    try:
        with torch.no_grad():
            ref = m.pure_model_forward(x)
    finally:
        m.HPARAM.USE_NATIVE_ENGINE = True
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        scale = max(1.0, ref[k].abs().max().item())
        err = (out["logits"][k] - ref[k]).abs().max().item()
        assert err <= 2e-4 * scale, (k, err, scale)
    cat = gtf.class_compression_fused(7, out["logits"])
    assert torch.equal(cat["mask"], out["categorical"]["mask"])
    for k in ("quaternion", "scales", "xy", "z"):
        assert torch.equal(cat[k], out["categorical"][k]), k
    assert set(out) == {"logits", "categorical", "aggregated"} and out["aggregated"] is None
    print("resnet50 B=32 plans:", eng.conv_plans())


def test_resnet50_pipeline_and_streamer(lib, dev):
    """The full PoseRegressor forward (aggregation, voting, RT) on a ResNet-50 encoder, and the streaming runtime against it."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.streaming import FrameStreamer
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.HV_NUM_OF_HYPOTHESES = 128
    hp.ENCODER = "resnet50"
    torch.manual_seed(0)
    m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).to(dev).eval()
    H, W = 96, 128
    x0 = synth.make_image(0, H, W)[None].to(dev)
    with torch.no_grad():
        full = m(x0)
    assert set(full) == {"logits", "categorical", "aggregated"}
    assert full["categorical"]["mask"].dtype == torch.int64 and tuple(full["categorical"]["mask"].shape) == (1, H, W)
    xs = [synth.make_image(i, H, W)[None].to(dev) for i in range(3)]
    cats = []
    for i in range(3):
        c, _ = synth.make_vote_frame(i, K=3, H=H, W=W, rmin=8, rmax=20)
        cats.append({k: v.to(dev) for k, v in c.items()})
    ref = []
    with torch.no_grad():
        for i in range(3):
            logits = m.pure_model_forward(xs[i])
            cat = m.class_compression(logits)
            torch.manual_seed(100 + i)
            ref.append((logits, cat, m.agg_hough_and_generate_RT(cats[i])))
    st = FrameStreamer(m)
    torch.manual_seed(99)
    st.prepare(xs[0], categorical_override=cats[0])
    tickets = []
    for i in range(3):
        torch.manual_seed(100 + i)
        tickets.append(st.submit(xs[i], categorical_override=cats[i]))
    for i in range(3):
        out = st.collect(tickets[i])
        for k in ("mask", "quaternion", "scales", "xy", "z"):
            a, b = out["logits"][k], ref[i][0][k]
            assert (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item()), (i, k)
        assert (out["categorical"]["mask"] != ref[i][1]["mask"]).float().mean().item() < 1e-3
        assert set(out["aggregated"]) == set(ref[i][2])
        for k, v in ref[i][2].items():
            assert torch.equal(out["aggregated"][k], v), (i, k)


def test_resnet50_training_step_native_vs_torch(lib, dev, monkeypatch):
    """Forward + backward of a small ResNet-50 model in training mode: native convolutions against the same model on torch's
    f32 kernels (train_conv.ENABLED = False), each against float64 — the bars of test_gpu_train.py's whole-network check."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet50"
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
        for name, child in list(mod.named_children()):
            if isinstance(child, torch.nn.ReLU):
                setattr(mod, name, torch.nn.Softplus())
    x = torch.stack([synth.make_image(i, 64, 96) for i in range(2)]).to(dev)
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
    assert used["fwd_native"] >= 100 and used["wgrad_native"] >= 45 and used["dgrad_native"] >= 40, used
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
