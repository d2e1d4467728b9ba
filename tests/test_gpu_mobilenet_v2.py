"""The MobileNetV2 encoder on the MI355X: the three kernels of csrc/mobilenet.hip (fpc_dwconv3x3, fpc_conv1x1_f32, fpc_stem3x3s2)
against float64 torch on the CPU at the kernel bar 2e-5 max(1, |ref|max), every case launched twice and bit-identical, outputs in
NaN-filled buffers between 64-float canaries; their refusals; the engine's mobilenet_v2 plan against the float64 CPU module path at
the network bar 1e-4 max(1, |ref|max) on c2 .. c5 and all five logits; graph replay and the streaming runtime bit for bit at full
size; and one training-mode step against torch's f32 kernels and float64."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RELU6 = 1           # the entries' `act`: 0 = none, 1 = ReLU6

# (B, Hi, Wi, C, stride): all halo; odd sizes (the clipped last window) at both strides; even sizes at stride 2 (no bottom / right
# padding is read); the widest channel count on the smallest real map; more pixels than one strip and row in both directions with C
# below a wave's width; the smallest C
DW_CASES = [(1, 1, 1, 32, 1), (3, 5, 7, 96, 1), (3, 5, 7, 96, 2), (2, 6, 8, 144, 2), (1, 2, 3, 960, 1), (2, 17, 33, 16, 1), (1, 9, 64, 4, 2)]
# (M as (B, H, W), Cin, Cout, act, residual): the smallest of everything; the first expand site; Cin % 16 != 0; a partial last channel
# tile with a residual; long K, few rows; the widest output; the t = 1 project site
PW_CASES = [((1, 1, 1), 8, 8, 0, False), ((3, 5, 7), 16, 96, RELU6, False), ((2, 9, 11), 24, 144, RELU6, False),
            ((2, 9, 11), 144, 24, 0, True), ((1, 2, 3), 960, 160, 0, True), ((1, 2, 3), 320, 1280, RELU6, False),
            ((2, 13, 13), 32, 16, 0, False)]
# The 1x1 kernel has two tile forms, picked by the shape alone (fpc_conv1x1_f32_form): 16 x 16 tiles where 32 x 32 ones would make
# fewer than 1024 waves — every case above — else 32 x 32 tiles with 1, 2, 3 or 5 channel tiles per wave (2048 waves left).  These
# cases sit on the other side of that threshold, one per form, with an odd row count and K loops of an even count, an odd count and
# none (tail steps only): (M, Cin, Cout, act, residual, form).  The last two straddle the threshold itself.
PW_FORM_CASES = [(32 * 1024 + 5, 72, 24, RELU6, False, 1), (32 * 2048 + 5, 40, 64, 0, True, 2), (32 * 2048 + 5, 40, 96, RELU6, False, 3),
                 (32 * 2048 + 5, 8, 160, 0, True, 5), (32 * 1023, 24, 8, 0, False, 0), (32 * 1023 + 1, 24, 8, 0, False, 1)]
STEM_CASES = [(1, 2, 2), (2, 6, 10), (1, 7, 9), (1, 32, 64)]


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


def _twice(dev, n, launch):
    """Two launches into fresh NaN-filled buffers with 64-float canaries around the n outputs: the canaries intact, nothing left
    unwritten, both runs the same bits.  Returns the first run's outputs (CPU, flat)."""
    outs = []
    for _ in range(2):
        buf = torch.full((n + 128,), float("nan"), device=dev)
        y = buf[64:64 + n]
        assert y.data_ptr() % 16 == 0
        assert launch(y.data_ptr()) == 0
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.isnan(host[:64]).all() and torch.isnan(host[64 + n:]).all(), "a canary was overwritten"
        outs.append(host[64:64 + n])
    assert not torch.isnan(outs[0]).any(), "unwritten outputs"
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def _bar(out, ref, what):
    err = (out.double() - ref).abs().max().item()
    print(what, "err", err, "ref max", ref.abs().max().item())
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (what, err)


@pytest.mark.parametrize("act", [RELU6, 0], ids=["relu6", "plain"])
@pytest.mark.parametrize("case", DW_CASES, ids=[f"B{b}-{h}x{w}-C{c}-s{s}" for b, h, w, c, s in DW_CASES])
def test_dwconv3x3_vs_float64(lib, dev, case, act):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, Hi, Wi, C, s = case
    g = torch.Generator().manual_seed(10 * DW_CASES.index(case) + act)
    x = torch.randn((B, C, Hi, Wi), generator=g)
    w = torch.randn((C, 1, 3, 3), generator=g)
    scale = (torch.rand(C, generator=g) + 0.5) * 4.0            # pre-activations of order ten: both clamps engage
    shift = torch.randn(C, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, s, 1, 1, C) * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
    assert (ref < 0).any() and (ref > 6).any()
    if act:
        ref = ref.clamp(0.0, 6.0)
    Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
    assert tuple(ref.shape) == (B, C, Ho, Wo)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, sd, hd = w.to(dev), scale.to(dev), shift.to(dev)
    out = _twice(dev, ref.numel(), lambda y: L.fpc_dwconv3x3(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y, B, Hi, Wi, C,
                                                             s, act, nat.stream()))
    out = out.view(B, Ho, Wo, C).permute(0, 3, 1, 2)
    _bar(out, ref, f"dwconv3x3 {case} act {act}")
    if act:
        assert (out == 0).any() and (out == 6).any() and out.max() <= 6 and out.min() >= 0
    else:
        assert out.min() < 0 and out.max() > 6                   # nothing is clamped


@pytest.mark.parametrize("case", PW_CASES + PW_FORM_CASES,
                         ids=[f"M{b}x{h}x{w}-{ci}to{co}-act{a}-res{int(r)}" for (b, h, w), ci, co, a, r in PW_CASES] +
                             [f"M{m}-{ci}to{co}-act{a}-res{int(r)}-form{f}" for m, ci, co, a, r, f in PW_FORM_CASES])
def test_conv1x1_f32_vs_float64(lib, dev, case):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    if len(case) == 6:
        M, Cin, Cout, act, has_res, form = case
        seed = 200 + PW_FORM_CASES.index(case)
    else:
        (B, H, W), Cin, Cout, act, has_res = case
        M, form, seed = B * H * W, 0, 100 + PW_CASES.index(case)
    assert L.fpc_conv1x1_f32_form(M, Cin, Cout) == form
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, Cin), generator=g)
    w = torch.randn((Cout, Cin, 1, 1), generator=g) / Cin ** 0.5
    scale = (torch.rand(Cout, generator=g) + 0.5) * 4.0
    shift = torch.randn(Cout, generator=g)
    res = torch.randn((M, Cout), generator=g)
    ref = x.double() @ w.double().view(Cout, Cin).t() * scale.double() + shift.double()
    if act:
        assert (ref < 0).any() and (ref > 6).any()
        ref = ref.clamp(0.0, 6.0)
    xd, wd, sd, hd, rd = (t.to(dev) for t in (x, w, scale, shift, res))

    def run(r):
        return _twice(dev, M * Cout, lambda y: L.fpc_conv1x1_f32(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), r, y, M, Cin,
                                                                 Cout, act, nat.stream())).view(M, Cout)
    plain = run(None)
    _bar(plain, ref, f"conv1x1_f32 {case}")
    if act:
        assert (plain == 0).any() and (plain == 6).any() and plain.max() <= 6 and plain.min() >= 0
    if has_res:
        with_res = run(rd.data_ptr())
        _bar(with_res, ref + res.double(), f"conv1x1_f32 {case} + res")
        assert not torch.equal(with_res, plain)


@pytest.mark.parametrize("B,Hi,Wi", STEM_CASES)
def test_stem3x3s2_vs_float64(lib, dev, B, Hi, Wi):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    g = torch.Generator().manual_seed(1000 + Hi * 100 + Wi)
    x = torch.randn((B, 3, Hi, Wi), generator=g)
    w = torch.randn((32, 3, 3, 3), generator=g) / 27 ** 0.5
    scale = (torch.rand(32, generator=g) + 0.5) * 4.0
    shift = torch.randn(32, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, 2, 1) * scale.double().view(1, 32, 1, 1) + shift.double().view(1, 32, 1, 1)
    assert (ref < 0).any() and (ref > 6).any()
    ref = ref.clamp(0.0, 6.0)
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    assert tuple(ref.shape) == (B, 32, Ho, Wo)
    if Hi % 2 == 0 and Wi % 2 == 0:      # the engine's own image
        x4 = torch.full((B, Hi, Wi, 4), float("nan"), device=dev)
        assert L.fpc_image_nhwc4(x.to(dev).data_ptr(), x4.data_ptr(), B, Hi, Wi, nat.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(x4[..., :3].cpu(), x.permute(0, 2, 3, 1)) and (x4[..., 3] == 0).all()
    else:
        x4 = torch.cat([x.permute(0, 2, 3, 1), torch.zeros(B, Hi, Wi, 1)], dim=3).contiguous().to(dev)
    wd, sd, hd = w.to(dev), scale.to(dev), shift.to(dev)
    out = _twice(dev, ref.numel(), lambda y: L.fpc_stem3x3s2(x4.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y, B, Hi, Wi, 32,
                                                             nat.stream()))
    out = out.view(B, Ho, Wo, 32).permute(0, 3, 1, 2)
    _bar(out, ref, f"stem3x3s2 {(B, Hi, Wi)}")
    assert (out == 0).any() and (out == 6).any() and out.max() <= 6 and out.min() >= 0


def test_refusals(lib, dev):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    s = nat.stream()
    p = lambda t: t.data_ptr()
    B, H, W, C = 2, 5, 7, 32
    x, y, res = (torch.zeros(B * H * W * 96 + 8, device=dev) for _ in range(3))
    w, scale, shift = torch.zeros(96 * 32 + 8, device=dev), torch.ones(96 + 8, device=dev), torch.zeros(96 + 8, device=dev)
    good = [p(x), p(w), p(scale), p(shift), p(y)]
    assert L.fpc_dwconv3x3(*good, B, H, W, C, 1, RELU6, s) == 0
    assert L.fpc_dwconv3x3(*good, B, H, W, C, 2, 0, s) == 0
    for bad in ((B, H, W, 6, 1, 0), (B, H, W, C, 3, 0), (0, H, W, C, 1, 0), (B, H, W, C, 1, 2)):
        assert L.fpc_dwconv3x3(*good, *bad, s) == -1, bad
    for i in range(5):
        args = list(good)
        args[i] = None
        assert L.fpc_dwconv3x3(*args, B, H, W, C, 1, 0, s) == -1, ("null", i)
        args[i] = good[i] + 4
        assert L.fpc_dwconv3x3(*args, B, H, W, C, 1, 0, s) == -1, ("misaligned", i)
    M = B * H * W
    good = [p(x), p(w), p(scale), p(shift), p(res), p(y)]
    assert L.fpc_conv1x1_f32(*good, M, 32, 96, 0, s) == 0
    assert L.fpc_conv1x1_f32(*good[:4], None, good[5], M, 32, 96, RELU6, s) == 0
    assert L.fpc_conv1x1_f32(*good, M, 32, 96, RELU6, s) == -1                    # a residual with an activation
    for bad in ((M, 12, 96, 0), (M, 32, 12, 0), (0, 32, 96, 0), (M, 32, 96, 2)):
        assert L.fpc_conv1x1_f32(*good, *bad, s) == -1, bad
    for i in range(6):
        args = list(good)
        args[i] = good[i] + 4
        assert L.fpc_conv1x1_f32(*args, M, 32, 96, 0, s) == -1, ("misaligned", i)
        if i != 4:
            args[i] = None
            assert L.fpc_conv1x1_f32(*args, M, 32, 96, 0, s) == -1, ("null", i)
    good = [p(x), p(w), p(scale), p(shift), p(y)]
    assert L.fpc_stem3x3s2(*good, B, H, W, 32, s) == 0
    assert L.fpc_stem3x3s2(*good, B, H, W, 64, s) == -1
    assert L.fpc_stem3x3s2(*good, 0, H, W, 32, s) == -1
    for i in range(5):
        args = list(good)
        args[i] = None
        assert L.fpc_stem3x3s2(*args, B, H, W, 32, s) == -1, ("null", i)
        args[i] = good[i] + 4
        assert L.fpc_stem3x3s2(*args, B, H, W, 32, s) == -1, ("misaligned", i)
    torch.cuda.synchronize()


def _model(lib, seed=0):
    """test_gpu_se.py's model on mobilenet_v2: random BatchNorm and GroupNorm statistics and affines."""
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "mobilenet_v2"
    hp.PERFORM_AGGREGATION = False
    torch.manual_seed(seed)
    m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    g = torch.Generator().manual_seed(seed + 1)
    for name, mod in m.named_modules():
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
    """(model, hp, x, float64 logits, float64 encoder features), computed once per configuration and left unchanged."""
    from fastposecnn_amd import synth
    key = (B, H, W)
    if key not in _REFS:
        m, hp = _model(lib)
        x = torch.stack([synth.make_image(i, H, W) for i in range(B)])
        ref_m = copy.deepcopy(m).double()
        ref_m.HPARAM = copy.copy(hp)
        ref_m.HPARAM.USE_NATIVE_ENGINE = False
        with torch.no_grad():
            _REFS[key] = (m, hp, x, ref_m.pure_model_forward(x.double()), ref_m.encoder(x.double()))
    return _REFS[key]


def _check(eng, logits, ref, feats, tol=1e-4):
    for name, f, C in zip(("c2", "c3", "c4", "c5"), feats[2:], (24, 32, 96, 1280)):
        got = eng.tensor(name).permute(0, 3, 1, 2).cpu().double()
        assert got.shape == f.shape and got.shape[1] == C, name
        err = (got - f).abs().max().item()
        print(name, "err", err, "ref max", f.abs().max().item())
        assert err <= tol * max(1.0, f.abs().max().item()), (name, err)
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = logits[k].cpu().double()
        assert got.shape == ref[k].shape, k
        err = (got - ref[k]).abs().max().item()
        print(k, "err", err, "ref max", ref[k].abs().max().item())
        assert err <= tol * max(1.0, ref[k].abs().max().item()), (k, err)


@pytest.mark.parametrize("split", ["default", "no-f16", "f32"])
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 96, 64), (3, 32, 32)])
def test_engine_vs_float64_cpu(lib, dev, B, H, W, split):
    m0, hp0, x, ref, feats = _float64(lib, B, H, W)
    m = copy.deepcopy(m0)
    hp = m.HPARAM = copy.copy(hp0)
    if split == "no-f16":
        hp.ENGINE_SPLIT_F16 = False
    if split == "f32":
        hp.ENGINE_SPLIT_PRECISION = False
    m = m.to(dev)
    with torch.no_grad():
        out = m(x.to(dev))
    assert m._engines, "the native engine did not run"
    eng = next(iter(m._engines.values()))
    _check(eng, out["logits"], ref, feats)
    plans = eng.conv_plans()
    assert len(plans) == 44 and [p[4] for p in plans[:4]] == [1280, 96, 32, 24]         # the decoders' sites alone
    if split == "f32":
        assert not any(p[2] >= 1000 for p in plans)                                      # level 0: f32 products only
    with pytest.raises(RuntimeError):
        eng.force_stem_pool(1)
    assert eng.force_fold(0) == 0
    assert eng.flops()[0] > 0


def test_fullsize_graph_and_streamer(lib, dev):
    """640 x 480, B = 1: against float64; three forwards of the graph-recorded engine on a side stream and one frame through the
    streaming runtime (the same plan on a stream of its own) return the plain launches' bits."""
    from fastposecnn_amd.streaming import FrameStreamer
    m0, hp0, x, ref, feats = _float64(lib, 1, 480, 640)
    m = copy.deepcopy(m0)
    m.HPARAM = copy.copy(hp0)
    m = m.to(dev)
    xd = x.to(dev)
    with torch.no_grad():
        out = m(xd)                                   # (the null stream: plain launches)
    torch.cuda.synchronize()
    assert m._engines
    eng = next(iter(m._engines.values()))
    _check(eng, out["logits"], ref, feats)
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
    print("mobilenet_v2 B=1 plans:", eng.conv_plans())


# The bias of a project BatchNorm shifts its block's output by a constant per channel.  That constant rides through the residual adds
# of the blocks behind it and dies at the first 1x1 convolution followed by a training-mode BatchNorm (which removes a per-channel
# constant exactly; a project output never feeds a padded depthwise convolution directly).  So the bias has a gradient only where
# residual adds alone carry it to a tapped feature level (c2 .. c4, read by the laterals): blocks 2-3, 4-6 and 11-13.  For blocks 1,
# 7-10 and 14-17 it has NONE: float64 returns 1e-17 there and f32 its rounding noise, and "relative to the parameter's own gradient"
# would compare noise with noise.  Derived from the module's residual flags and smp's stage ends, not from a run.
def _zero_grad_biases(encoder):
    taps = {s - 1 for s in encoder.STAGES[:-1]}                    # features.1 / 3 / 6 / 13 (features.18 has its own BatchNorm)
    out = set()
    for i in range(1, 18):
        j, alive = i, i in taps
        while not alive and j + 1 < 18 and encoder.features[j + 1].use_res_connect:
            j += 1
            alive = j in taps
        if not alive or i == 1:                                     # (level 1, behind features.1, feeds no lateral)
            out.add(f"encoder.features.{i}.conv.{len(encoder.features[i].conv) - 1}.bias")
    return out


def test_training_step_native_vs_torch(lib, dev, monkeypatch):
    """Forward + backward of a small mobilenet_v2 model in training mode: the native convolutions and BatchNorms against the same
    model on torch's f32 kernels, each against float64 — test_gpu_se.py's form and bars.  ReLU and ReLU6 are swapped for Softplus
    (the kinks at 0 and 6 would make f32 and float64 gradients disagree arbitrarily); the depthwise convolutions are torch's on
    both sides."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "mobilenet_v2"
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    swapped = 0
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
        for name, child in list(mod.named_children()):
            if isinstance(child, (torch.nn.ReLU, torch.nn.ReLU6)):
                setattr(mod, name, torch.nn.Softplus())
                swapped += isinstance(child, torch.nn.ReLU6)
    assert swapped == 35                               # the stem, 16 expand, 17 depthwise and the last 1x1
    x = torch.stack([synth.make_image(i, 64, 64) for i in range(2)]).to(dev)
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
    print("mobilenet_v2 training step: counters", used)
    assert used["fwd_native"] > 0, used                # the dense sites with Cin % 32 == 0
    assert unused["fwd_native"] == 0
    assert abs(ln - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in orf:
        assert (on[k] - orf[k]).abs().max().item() <= 1e-4 * max(1.0, orf[k].abs().max().item()), k
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert set(gn) == set(gr) == set(names), "a parameter without a gradient"
    assert sum(n.startswith("encoder.") for n in names) == 156            # 52 convolutions and their BatchNorms' weight and bias
    assert "encoder.features.1.conv.0.0.weight" in gn and "encoder.features.18.0.weight" in gn
    err_n = err_t = 0.0
    worst = None
    ZERO_GRAD = _zero_grad_biases(model.encoder)
    assert sorted(int(n.split(".")[2]) for n in ZERO_GRAD) == [1, 7, 8, 9, 10, 14, 15, 16, 17]
    for n in gr:
        ref_n = n
        if n in ZERO_GRAD:      # held against the scale of the same BatchNorm's weight gradient: its own is zero
            ref_n = n[:-len("bias")] + "weight"
            assert gr[n].abs().max().item() <= 1e-9 * gr[ref_n].abs().max().item(), n
        scale = max(gr[ref_n].abs().max().item(), 1e-12)
        e = (gn[n] - gr[n]).abs().max().item() / scale
        if e > err_n:
            worst = (n, scale)
        err_n = max(err_n, e)
        err_t = max(err_t, (gt[n] - gr[n]).abs().max().item() / scale)
    print("mobilenet_v2 training step: err native", err_n, "torch", err_t, "worst", worst)
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)
