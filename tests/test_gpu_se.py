"""The SE-ResNet encoders on the MI355X: the squeeze-and-excitation kernels of csrc/se.hip (k_se_pool + k_se_excite through
fpc_se_gate, k_se_scale_add_relu) and the ceil-mode stem pool against float64 torch on the CPU at the kernel bar
2e-5 max(1, |ref|max), every case launched twice and bit-identical; the engine's se_resnet50 / se_resnet101 plans against the float64
CPU module path at the network bar 1e-4, graph replay and the streaming runtime bit for bit, and one training-mode step."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, H, W, C, R): one pixel; odd sizes, three frames; the widest stage (C / 4 > 256 lanes: several quads per thread, 5 slabs);
# more pixels than one slab and an odd count (3 slabs); two thread rows, 5 slabs; C / R = 2: fc2's rows are not 16-byte aligned
SHAPES = [(1, 1, 1, 64, 16), (3, 5, 7, 256, 16), (2, 15, 20, 2048, 16), (1, 37, 41, 128, 8), (2, 9, 64, 512, 16), (2, 3, 3, 64, 32)]
IDS = [f"B{b}-{h}x{w}-C{c}-R{r}" for b, h, w, c, r in SHAPES]


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


def _gate_inputs(case, mode):
    """x NHWC (randn + 1: a mean far from zero; mode "zero": frame 0 all zeros), fc1 / fc2 weights of unit-scale products, biases
    of order one (an ignored bias moves the gate by ~0.2); mode "sat": b2 = +100 on even channels, -100 on odd ones."""
    B, H, W, C, R = case
    g = torch.Generator().manual_seed(100 * SHAPES.index(case) + {"plain": 0, "zero": 1, "sat": 2}[mode])
    x = torch.randn((B, H, W, C), generator=g) + 1.0
    if mode == "zero":
        x[0].zero_()
    Cr = C // R
    w1 = torch.randn((Cr, C), generator=g) / C ** 0.5
    b1 = torch.randn(Cr, generator=g)
    w2 = torch.randn((C, Cr), generator=g) / Cr ** 0.5
    b2 = torch.randn(C, generator=g)
    if mode == "sat":
        b2 = torch.where(torch.arange(C) % 2 == 0, 100.0, -100.0)
    return x, w1, b1, w2, b2


def _gate_ref(x, w1, b1, w2, b2):
    m = x.double().mean(dim=(1, 2))
    h = (m @ w1.double().t() + b1.double()).relu()
    return torch.sigmoid(h @ w2.double().t() + b2.double())


def _gate(dev, x, w1, b1, w2, b2, R):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, H, W, C = x.shape
    xd, w1d, b1d, w2d, b2d = (t.contiguous().to(dev) for t in (x, w1, b1, w2, b2))
    n = L.fpc_se_scratch_floats(B, H, W, C)
    assert n == B * L.fpc_se_pool_slabs(H, W, C) * C > 0
    scratch = torch.full((n,), float("nan"), device=dev)
    gate = torch.full((B, C), float("nan"), device=dev)
    rc = L.fpc_se_gate(xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), gate.data_ptr(),
                       scratch.data_ptr(), B, H, W, C, R, nat.stream())
    torch.cuda.synchronize()
    return rc, gate.cpu()


@pytest.mark.parametrize("mode", ["plain", "zero", "sat"])
@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_se_gate_vs_float64(lib, dev, case, mode):
    from fastposecnn_amd import _native as nat
    B, H, W, C, R = case
    if case == (1, 37, 41, 128, 8):
        assert nat.lib().fpc_se_pool_slabs(H, W, C) > 1
    x, w1, b1, w2, b2 = _gate_inputs(case, mode)
    rc, out = _gate(dev, x, w1, b1, w2, b2, R)
    assert rc == 0
    assert torch.isfinite(out).all(), "NaN or unwritten gate"
    ref = _gate_ref(x, w1, b1, w2, b2)
    err = (out.double() - ref).abs().max().item()
    print("se_gate", case, mode, "err", err)
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err
    if mode == "sat":
        assert torch.equal(out[:, 0::2], torch.ones(B, C // 2)) and torch.equal(out[:, 1::2], torch.zeros(B, C // 2))
    if mode == "zero":       # the gate of the zero frame is sigmoid(fc2(relu(b1)) + b2): the biases alone
        only_bias = torch.sigmoid(b1.double().relu() @ w2.double().t() + b2.double())
        assert (out[0].double() - only_bias).abs().max().item() <= 2e-5
    rc2, out2 = _gate(dev, x, w1, b1, w2, b2, R)
    assert rc2 == 0 and torch.equal(out, out2)


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_se_scale_add_relu_vs_float64(lib, dev, case, inplace):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, H, W, C, _ = case
    g = torch.Generator().manual_seed(7 + SHAPES.index(case))
    x = torch.randn((B, H, W, C), generator=g)
    res = torch.randn((B, H, W, C), generator=g)
    gate = torch.rand((B, C), generator=g)
    ref = (x.double() * gate.double().view(B, 1, 1, C) + res.double()).relu()
    n = x.numel()
    outs = []
    for _ in range(2):
        buf = torch.full((n + 128,), float("nan"), device=dev)       # NaN canaries 64 floats before and after y
        y = buf[64:64 + n]
        assert y.data_ptr() % 16 == 0
        resd, gd = res.to(dev), gate.to(dev)
        if inplace:
            y.copy_(x.reshape(-1).to(dev))
            xp = y.data_ptr()
        else:
            xd = x.to(dev)
            xp = xd.data_ptr()
        rc = L.fpc_se_scale_add_relu(xp, gd.data_ptr(), resd.data_ptr(), y.data_ptr(), B, H, W, C, nat.stream())
        torch.cuda.synchronize()
        assert rc == 0
        host = buf.cpu()
        assert torch.isnan(host[:64]).all() and torch.isnan(host[64 + n:]).all(), "a canary was overwritten"
        outs.append(host[64:64 + n].view(B, H, W, C))
    assert not torch.isnan(outs[0]).any(), "unwritten outputs"
    err = (outs[0].double() - ref).abs().max().item()
    print("se_scale", case, inplace, "err", err)
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err
    assert (outs[0] >= 0).all() and (outs[0] == 0).any()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("B,Hi,Wi,C", [(1, 8, 12, 64), (2, 7, 9, 64), (1, 32, 48, 64)])
def test_maxpool_ceil_equals_torch(lib, dev, B, Hi, Wi, C):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    g = torch.Generator().manual_seed(Hi * 100 + Wi)
    x = torch.randn((B, C, Hi, Wi), generator=g)
    ref = F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    assert tuple(ref.shape) == (B, C, Hi // 2, Wi // 2)
    assert not torch.equal(ref, F.max_pool2d(x, 3, 2, 1)[:, :, :Hi // 2, :Wi // 2])
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    outs = []
    for _ in range(2):
        y = torch.full((B, Hi // 2, Wi // 2, C), float("nan"), device=dev)
        assert L.fpc_maxpool3x3s2_ceil_fwd(xd.data_ptr(), y.data_ptr(), B, Hi, Wi, C, nat.stream()) == 0
        torch.cuda.synchronize()
        outs.append(y.permute(0, 3, 1, 2).cpu())
    assert torch.equal(outs[0], ref) and torch.equal(outs[1], ref)


def test_refusals(lib, dev):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    s = nat.stream()
    B, H, W, C, R = 2, 5, 7, 128, 16
    big = torch.zeros(B * H * W * C + 8, device=dev)
    x, res, y = big[:-8], torch.zeros(B * H * W * C + 8, device=dev), torch.zeros(B * H * W * C + 8, device=dev)
    w1, b1, w2, b2 = (torch.zeros(n + 8, device=dev) for n in (C // R * C, C // R, C * C // R, C))
    gate, scratch = torch.zeros(B * C + 8, device=dev), torch.zeros(L.fpc_se_scratch_floats(B, H, W, C) + 8, device=dev)
    p = lambda t: t.data_ptr()
    good = [p(x), p(w1), p(b1), p(w2), p(b2), p(gate), p(scratch)]
    assert L.fpc_se_gate(*good, B, H, W, C, R, s) == 0
    for C_bad in (96, 32, 0, 100):
        assert L.fpc_se_gate(*good, B, H, W, C_bad, 16, s) == -1, C_bad
    for R_bad in (0, -1, 3, 24, 256):
        assert L.fpc_se_gate(*good, B, H, W, C, R_bad, s) == -1, R_bad
    assert L.fpc_se_gate(*good, 0, H, W, C, R, s) == -1
    for i in range(len(good)):
        args = list(good)
        args[i] = None
        assert L.fpc_se_gate(*args, B, H, W, C, R, s) == -1, ("null", i)
        args[i] = good[i] + 4
        assert L.fpc_se_gate(*args, B, H, W, C, R, s) == -1, ("misaligned", i)
    good = [p(x), p(gate), p(res), p(y)]
    assert L.fpc_se_scale_add_relu(*good, B, H, W, C, s) == 0
    assert L.fpc_se_scale_add_relu(*good, B, H, W, 96, s) == -1
    for i in range(len(good)):
        args = list(good)
        args[i] = None
        assert L.fpc_se_scale_add_relu(*args, B, H, W, C, s) == -1, ("null", i)
        args[i] = good[i] + 8
        assert L.fpc_se_scale_add_relu(*args, B, H, W, C, s) == -1, ("misaligned", i)
    assert L.fpc_maxpool3x3s2_ceil_fwd(p(x), p(y), 1, 8, 8, 64, s) == 0
    assert L.fpc_maxpool3x3s2_ceil_fwd(p(x), p(y), 1, 8, 8, 96, s) == -1
    assert L.fpc_maxpool3x3s2_ceil_fwd(p(x), p(y), 1, 1, 8, 64, s) == -1
    assert L.fpc_maxpool3x3s2_ceil_fwd(None, p(y), 1, 8, 8, 64, s) == -1
    assert L.fpc_maxpool3x3s2_ceil_fwd(p(x), None, 1, 8, 8, 64, s) == -1
    assert L.fpc_maxpool3x3s2_ceil_fwd(p(x) + 4, p(y), 1, 8, 8, 64, s) == -1
    assert L.fpc_maxpool3x3s2_ceil_fwd(p(x), p(y) + 4, 1, 8, 8, 64, s) == -1
    torch.cuda.synchronize()


def _model(lib, encoder, seed=0):
    """test_gpu_bottleneck.py's model: random BatchNorm statistics and affines, and here random SE biases too (gates spread over
    (0, 1) instead of sitting near 0.5)."""
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = encoder
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
        if name.endswith("se_module.fc1") or name.endswith("se_module.fc2"):
            mod.bias.data.copy_(torch.randn(mod.out_channels, generator=g))
    return m.eval(), hp


_REFS = {}


def _float64(lib, encoder, B, H, W):
    """(model, hp, x, float64 logits, float64 encoder features), computed once per configuration and left unchanged."""
    from fastposecnn_amd import synth
    key = (encoder, B, H, W)
    if key not in _REFS:
        m, hp = _model(lib, encoder)
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


@pytest.mark.parametrize("split", ["default", "no-f16", "f32"])
@pytest.mark.parametrize("encoder,B,H,W", [("se_resnet50", 2, 64, 96), ("se_resnet101", 1, 96, 64)])
def test_engine_vs_float64_cpu(lib, dev, encoder, B, H, W, split):
    m0, hp0, x, ref, feats = _float64(lib, encoder, B, H, W)
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
    blocks = {"se_resnet50": 16, "se_resnet101": 33}[encoder]
    assert sum(1 for p in plans[:1 + 3 * blocks + 4] if p[4] == 9 * p[3]) == blocks          # every conv2 a 3x3 / stride-1 site
    if split == "f32":
        assert not any(p[2] >= 4000 for p in plans)                       # level 0: f32 products only
    assert plans[0][2] != 3100                                            # the fused stem + pad-1 pool is never chosen ...
    with pytest.raises(RuntimeError):
        eng.force_stem_pool(1)                                            # ... and cannot be forced
    assert eng.flops()[0] > 0


def test_fullsize_graph_and_streamer(lib, dev):
    """se_resnet50 at 640 x 480, B = 1: against float64; three forwards of the graph-recorded engine and one frame through the
    streaming runtime (the same plan on a stream of its own) return the plain launches' bits."""
    from fastposecnn_amd.streaming import FrameStreamer
    m0, hp0, x, ref, feats = _float64(lib, "se_resnet50", 1, 480, 640)
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
    print("se_resnet50 B=1 plans:", eng.conv_plans())


def test_training_step_native_vs_torch(lib, dev, monkeypatch):
    """Forward + backward of a small se_resnet50 model in training mode: the native convolutions and BatchNorms against the same
    model on torch's f32 kernels, each against float64 — test_gpu_bottleneck.py's form and bars.  fc1 / fc2 and the ceil-mode pool
    are torch modules on both sides."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "se_resnet50"
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
    assert set(gn) == set(gr) and any(n.endswith("se_module.fc1.bias") for n in gn)
    err_n = err_t = 0.0
    for n in gr:
        scale = max(gr[n].abs().max().item(), 1e-12)
        err_n = max(err_n, (gn[n] - gr[n]).abs().max().item() / scale)
        err_t = max(err_t, (gt[n] - gr[n]).abs().max().item() / scale)
    print("se_resnet50 training step: err native", err_n, "torch", err_t)
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)
