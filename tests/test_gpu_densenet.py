"""The DenseNet encoders on the MI355X: the kernels behind fpc_dense_pw, fpc_dense_conv3x3, fpc_dense_norm_pool and fpc_dense_place
(csrc/densenet.hip) against float64 torch on the CPU at the kernel bar 2e-5 max(1, |ref|max), every case launched twice and
bit-identical, outputs in NaN-filled buffers between 64-float canaries, everything a pitched kernel must not write pre-filled with a
pattern and compared bit for bit; whole-number operands bit for bit; the engine's densenet121 / 169 / 201 plans against the float64
CPU module at the network bar 1e-4 max(1, |ref|max) on c2 .. c5 and all five logits; graph replay and the streaming runtime bit for
bit at full size; and one training-mode step against torch's f32 kernels and float64."""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import _densenet_model as D
from _densenet_kernels import NAN, _bar, _conv_run, _pitched, _pw_operands, _pw_ref, _twice

pytestmark = pytest.mark.gpu

PW_M = [1, 30, 33, 300]                                  # one row; under / over one 32-row tile; 19 tiles of 16 with a ragged last one
PW_K = [(64, 64), (96, 256), (160, 512), (1024, 1024), (1920, 1920)]      # (K, ldi): dense, and prefixes of a wider row
CONV_SHAPES = [(1, 1, 1), (2, 2, 2), (1, 3, 5), (2, 7, 9), (1, 15, 20), (1, 8, 40)]
CONV_SLICES = [(0, 32), (64, 256), (224, 256)]           # (c0, ldo): dense, the middle and the last slice of a wider pixel


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


# ---------------------------------------------------------------------------------------------------------------- fpc_dense_pw

def _pw_sweep(dev, M, K, ldi, whole, seed):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    g = torch.Generator().manual_seed(seed)
    x, xin, s1, t1, w, s2, t2 = _pw_operands(g, M, K, ldi, whole)
    xd, s1d, t1d, s2d, t2d = (t.to(dev) for t in (xin, s1, t1, s2, t2))
    for Cout in (128, 32):
        wd = w[:Cout].contiguous().to(dev)
        assert L.fpc_dense_pw_form(M, K, Cout) == 0            # few rows: the shape's own form is the 16 x 16 one; 1 is forced below
        for ldo, pre, act, form in itertools.product((Cout, 256), (0, 1), (0, 1), (0, 1)):
            ref = _pw_ref(x, s1, t1, w, s2, t2, Cout, pre, act)
            out = _twice(dev, _pitched(M, ldo, 0, Cout), lambda y: L.fpc_dense_pw(
                xd.data_ptr(), s1d.data_ptr() if pre else None, t1d.data_ptr() if pre else None, wd.data_ptr(), s2d.data_ptr(), t2d.data_ptr(),
                y, M, K, Cout, ldi, ldo, act, form, nat.stream())).view(M, ldo)[:, :Cout]
            assert torch.isfinite(out).all(), "read behind channel K"
            what = f"dense_pw M{M} K{K}/{ldi} Cout{Cout}/{ldo} pre{pre} act{act} form{form}"
            if whole:
                assert torch.equal(out.double(), ref), what
            else:
                _bar(out, ref, what)
                if act:
                    assert out.min() >= 0.0


@pytest.mark.parametrize("K,ldi", PW_K)
@pytest.mark.parametrize("M", PW_M)
def test_pw_vs_float64(lib, dev, M, K, ldi):
    _pw_sweep(dev, M, K, ldi, False, 100 * M + K)


@pytest.mark.parametrize("K,ldi", [(96, 256), (1920, 1920)])
@pytest.mark.parametrize("M", [33, 300])
def test_pw_whole_numbers_bit_for_bit(lib, dev, M, K, ldi):
    """Small whole numbers: pre(v) <= 11, every product and every partial sum (|.| <= 1920 x 11 x 2 < 2^24) is exact in f32, so both
    forms equal float64 bit for bit whatever their summation orders."""
    _pw_sweep(dev, M, K, ldi, True, 7 * M + K)


def test_pw_forms_by_shape(lib, dev):
    """The shape's own form (form = -1): 16 x 16 tiles on a deep map, 32 x 32 tiles from 1024 tiles on; each the forced form's bits."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    for M, K, Cout, want in ((300, 1024, 128, 0), (32768, 64, 32, 1), (32736, 64, 32, 0), (8192, 64, 128, 1), (19200, 256, 128, 1)):
        assert L.fpc_dense_pw_form(M, K, Cout) == want, (M, K, Cout)
    for M, K, Cout, want in ((300, 1024, 128, 0), (32768, 64, 32, 1)):
        g = torch.Generator().manual_seed(M)
        x, xin, s1, t1, w, s2, t2 = _pw_operands(g, M, K, K, False)
        xd, s1d, t1d, wd, s2d, t2d = (t.to(dev) for t in (xin, s1, t1, w[:Cout].contiguous(), s2, t2))
        run = lambda form: _twice(dev, _pitched(M, Cout, 0, Cout), lambda y: L.fpc_dense_pw(
            xd.data_ptr(), s1d.data_ptr(), t1d.data_ptr(), wd.data_ptr(), s2d.data_ptr(), t2d.data_ptr(), y, M, K, Cout, K, Cout, 1, form,
            nat.stream())).view(M, Cout)
        auto = run(-1)
        _bar(auto, _pw_ref(x, s1, t1, w, s2, t2, Cout, 1, 1), f"dense_pw by shape M{M}")
        assert torch.equal(auto, run(want))


# ----------------------------------------------------------------------------------------------------------- fpc_dense_conv3x3

@pytest.mark.parametrize("form", [0, 1], ids=["split", "tile"])
@pytest.mark.parametrize("c0,ldo", CONV_SLICES)
@pytest.mark.parametrize("B,H,W", CONV_SHAPES)
def test_conv3x3_vs_float64(lib, dev, B, H, W, c0, ldo, form):
    from fastposecnn_amd import _native as nat
    assert nat.lib().fpc_dense_conv3x3_form(B, H, W) == 0
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B)
    x = torch.randn((B, 128, H, W), generator=g)
    w = torch.randn((32, 128, 3, 3), generator=g) * 2.0 / 1152 ** 0.5
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    out = _conv_run(dev, x, w, c0, ldo, form)
    _bar(out, ref, f"dense_conv3x3 {(B, H, W)} c0 {c0}/{ldo} form{form}")
    if form == 0:
        assert torch.equal(out, _conv_run(dev, x, w, c0, ldo, -1))      # the shape's own form


def test_conv3x3_forms_by_shape(lib):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    # one wave per 64 pixels from 1024 waves on; 160 x 120 and every deeper map of one frame run the split form
    for B, H, W, want in ((1, 120, 160, 0), (1, 30, 40, 0), (1, 15, 20, 0), (32, 120, 160, 1), (32, 30, 40, 0), (1, 256, 256, 1), (1, 256, 255, 0)):
        assert L.fpc_dense_conv3x3_form(B, H, W) == want, (B, H, W)


@pytest.mark.parametrize("form", [0, 1], ids=["split", "tile"])
def test_conv3x3_one_hot_pixel_returns_the_flipped_taps(lib, dev, form):
    """One pixel set to 1 in one channel, whole-number weights: the neighbour at (dh, dw) holds w[n][c][1 - dh][1 - dw] bit for bit,
    everything further away 0 — a wrong pad or tap order cannot hide in a tolerance."""
    B, H, W, c, h0, w0 = 2, 7, 9, 77, 3, 8                   # (the pixel on the right edge: its right neighbours are padding)
    g = torch.Generator().manual_seed(5)
    w = torch.randint(-9, 10, (32, 128, 3, 3), generator=g).float()
    x = torch.zeros((B, 128, H, W))
    x[1, c, h0, w0] = 1.0
    out = _conv_run(dev, x, w, 64, 256, form)
    want = torch.zeros((B, 32, H, W))
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            if 0 <= h0 + dh < H and 0 <= w0 + dw < W:
                want[1, :, h0 + dh, w0 + dw] = w[:, c, 1 - dh, 1 - dw]
    assert torch.equal(out, want)
    assert torch.equal(out.double(), F.conv2d(x.double(), w.double(), None, 1, 1))


@pytest.mark.parametrize("form", [0, 1], ids=["split", "tile"])
@pytest.mark.parametrize("B,H,W", [(2, 7, 9), (1, 8, 40)])
def test_conv3x3_whole_numbers_bit_for_bit(lib, dev, B, H, W, form):
    g = torch.Generator().manual_seed(H)
    x = torch.randint(-4, 5, (B, 128, H, W), generator=g).float()
    w = torch.randint(-3, 4, (32, 128, 3, 3), generator=g).float()      # |sum| <= 1152 x 12 < 2^24
    assert torch.equal(_conv_run(dev, x, w, 224, 256, form).double(), F.conv2d(x.double(), w.double(), None, 1, 1))


# ------------------------------------------------------------------------------------------- fpc_dense_norm_pool, fpc_dense_place

@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B,H,W,C,pool", [(2, 2, 2, 64, True), (1, 6, 10, 256, True), (1, 30, 40, 1024, True), (1, 3, 5, 64, False),
                                          (1, 15, 20, 1024, False)])
def test_norm_pool(lib, dev, B, H, W, C, pool, act):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    g = torch.Generator().manual_seed(H * W + C + act)
    x = torch.randn((B, H, W, C), generator=g)
    s, t = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    ref = x.double() * s.double() + t.double()
    if act:
        ref = ref.clamp_min(0.0)
    xd, sd, td = x.to(dev), s.to(dev), t.to(dev)
    n, npool = x.numel(), x.numel() // 4 if pool else 0
    # skip and pooled in ONE canaried buffer: skip, 64 floats of pattern between them, pooled
    pre = torch.full((n + 64 + npool,), NAN)
    pre[n:n + 64] = torch.arange(64).float()
    body = _twice(dev, pre, lambda y: L.fpc_dense_norm_pool(xd.data_ptr(), sd.data_ptr(), td.data_ptr(), y, y + 4 * (n + 64) if pool else None,
                                                            B, H, W, C, act, nat.stream()))
    skip = body[:n].view(B, H, W, C)
    _bar(skip, ref, f"dense_norm_pool {(B, H, W, C)} act{act}")
    assert (skip.min() >= 0.0) if act else (skip.min() < -0.5)
    if pool:
        pooled = body[n + 64:].view(B, H // 2, W // 2, C)
        want = 0.25 * ((skip[:, 0::2, 0::2] + skip[:, 0::2, 1::2]) + (skip[:, 1::2, 0::2] + skip[:, 1::2, 1::2]))      # f32, the stated order
        assert torch.equal(pooled, want)


@pytest.mark.parametrize("M,ld", [(1, 64), (35, 256), (4800, 256)])
def test_place(lib, dev, M, ld):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    x = torch.randn((M, 64), generator=torch.Generator().manual_seed(M))
    xd = x.to(dev)
    out = _twice(dev, _pitched(M, ld, 0, 64), lambda y: L.fpc_dense_place(xd.data_ptr(), y, M, 64, ld, nat.stream())).view(M, ld)
    assert torch.equal(out[:, :64].view(torch.int32), x.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the engine

_REFS = {}


def _float64(lib, encoder, B, H, W):
    """(model, hp, x, float64 logits, float64 encoder features), computed once per configuration and left unchanged."""
    key = (encoder, B, H, W)
    if key not in _REFS:
        m, hp = D.model(lib, encoder)      # (the draw tests/test_densenet_encoder.py holds to a quarter of the network bar in torch's own f32)
        x = D.images(B, H, W)
        ref_m = copy.deepcopy(m).double()
        ref_m.HPARAM = copy.copy(hp)
        ref_m.HPARAM.USE_NATIVE_ENGINE = False
        with torch.no_grad():
            _REFS[key] = (m, hp, x, ref_m.pure_model_forward(x.double()), ref_m.encoder(x.double()))
    return _REFS[key]


def _check(eng, logits, ref, feats, channels, tol=1e-4):
    for name, f, C in zip(("c2", "c3", "c4", "c5"), feats[2:], channels):
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


def _engine_case(lib, dev, encoder, channels, B, H, W, split):
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
    _check(eng, out["logits"], ref, feats, channels)
    assert feats[5].min() < 0                                                            # norm5's output is not clamped
    plans = eng.conv_plans()
    # the stem and the decoders' sites alone: the dense ops are not convolution sites
    assert len(plans) == 45 and plans[0][3:] == (64, 7 * 4 * 8) and [p[4] for p in plans[1:5]] == list(channels[::-1])
    if split == "f32":
        assert not any(p[2] >= 1000 for p in plans)                                      # level 0: f32 products only
    with pytest.raises(RuntimeError):
        eng.force_fold(1)
    assert eng.force_fold(0) == 0
    assert eng.flops()[0] > 0
    return eng


@pytest.mark.parametrize("split", ["default", "no-f16", "f32"])
@pytest.mark.parametrize("B,H,W", D.SMALL_SHAPES)
def test_engine_vs_float64_cpu(lib, dev, B, H, W, split):
    """densenet121; at 32 x 32 block 4 runs on a 1 x 1 map."""
    eng = _engine_case(lib, dev, "densenet121", (256, 512, 1024, 1024), B, H, W, split)
    if (H, W) == (32, 32):
        assert tuple(eng.tensor("c5").shape) == (3, 1, 1, 1024)
    if split == "default":
        assert eng.force_direct_h3(1) == 0                                               # (level 3: no site has that form's image)


@pytest.mark.parametrize("encoder,channels", [("densenet169", (256, 512, 1280, 1664)), ("densenet201", (256, 512, 1792, 1920))])
def test_engine_deeper_variants_vs_float64_cpu(lib, dev, encoder, channels):
    _engine_case(lib, dev, encoder, channels, 1, 64, 64, "default")


def test_fullsize_graph_and_streamer(lib, dev):
    """640 x 480, B = 1, densenet121: against float64; three forwards of the graph-recorded engine on a side stream and one frame
    through the streaming runtime (the same plan on a stream of its own) return the plain launches' bits."""
    from fastposecnn_amd.streaming import FrameStreamer
    m0, hp0, x, ref, feats = _float64(lib, "densenet121", 1, 480, 640)
    m = copy.deepcopy(m0)
    m.HPARAM = copy.copy(hp0)
    m = m.to(dev)
    xd = x.to(dev)
    with torch.no_grad():
        out = m(xd)                                   # (the null stream: plain launches)
    torch.cuda.synchronize()
    assert m._engines
    eng = next(iter(m._engines.values()))
    _check(eng, out["logits"], ref, feats, (256, 512, 1024, 1024))
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
    print("densenet121 B=1 plans:", eng.conv_plans())


def test_training_step_native_vs_torch(lib, dev, monkeypatch):
    """Forward + backward of a small densenet121 model in training mode: the native convolutions and BatchNorms against the same
    model on torch's f32 kernels, each against float64 — test_gpu_efficientnet_b0.py's form and bars.  Every ReLU is swapped for
    Softplus (its kink at 0 would make f32 and float64 gradients disagree arbitrarily); the concatenation and the pools are torch's
    on both sides.  No gradient is structurally zero here: every convolution is bias-free, and every BatchNorm's bias passes through
    its own activation (norm1 / norm2 / norm0 / a transition's norm) or straight into the p5 lateral (norm5) before the next
    normalisation can remove a per-channel constant — read off DenseLayer / Transition / DenseNetEncoder.forward, not from a run."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "densenet121"
    # a plan cache of this test's own: the front end keeps the form it timed fastest per convolution shape for the whole process, and
    # DenseNet's transitions share shapes with other encoders' 1x1 sites — what this test times must not decide what later tests run
    monkeypatch.setattr(train_conv, "_plan_cache", {})
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
        for name, child in list(mod.named_children()):
            if isinstance(child, (torch.nn.ReLU, torch.nn.ReLU6)):
                setattr(mod, name, torch.nn.Softplus())
    assert not any(isinstance(mod, torch.nn.ReLU) for mod in model.modules())            # every ReLU is a named child
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
    print("densenet121 training step: counters", used)
    assert used["fwd_native"] > 0, used
    assert unused["fwd_native"] == 0
    assert abs(ln - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in orf:
        assert (on[k] - orf[k]).abs().max().item() <= 1e-4 * max(1.0, orf[k].abs().max().item()), k
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert set(gn) == set(gr) == set(names), "a parameter without a gradient"
    # conv0 + norm0, 58 layers of two convolutions and two BatchNorms, three transitions of one each, norm5
    assert sum(n.startswith("encoder.") for n in names) == 3 + 58 * 6 + 3 * 3 + 2
    err_n = err_t = 0.0
    worst = None
    for n in gr:
        scale = max(gr[n].abs().max().item(), 1e-12)
        e = (gn[n] - gr[n]).abs().max().item() / scale
        if e > err_n:
            worst = (n, scale)
        err_n = max(err_n, e)
        err_t = max(err_t, (gt[n] - gr[n]).abs().max().item() / scale)
    print("densenet121 training step: err native", err_n, "torch", err_t, "worst", worst)
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)
