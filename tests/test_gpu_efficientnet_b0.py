"""The EfficientNet-B0 encoder on the MI355X: the kernels behind fpc_mbconv_dw, fpc_mbconv_gate, fpc_mbconv_pw and fpc_mbconv_stem
(csrc/efficientnet.hip and the gated / swish instantiations of csrc/mobilenet.hip) against float64 torch on the CPU at the kernel bar
2e-5 max(1, |ref|max), every case launched twice and bit-identical, outputs in NaN-filled buffers between 64-float canaries; integer
operands bit for bit; the engine's efficientnet-b0 plan against the float64 CPU module path at the network bar 1e-4 max(1, |ref|max)
on c2 .. c5 and all five logits; graph replay and the streaming runtime bit for bit at full size; and one training-mode step against
torch's f32 kernels and float64."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NONE, RELU6, SWISH = 0, 1, 2           # the entries' `act`
ENCODER = "efficientnet-b0"

# (B, Hi, Wi, C): a map smaller than the window, every tap padding somewhere; W neither a strip multiple nor wider than two strips; a
# real site with C / 4 = 36; the widest channel count on a narrow map
DW_CASES = [(2, 2, 2, 4), (1, 6, 10, 32), (3, 30, 40, 144), (1, 16, 4, 1152)]
# (B, H, W, C, Cs): the widest gate on the deepest map (C / 4 > 256: a thread walks two quads); one pixel; C / 4 = 36 lanes and seven
# thread rows; the most slabs; a hidden width of 1 on an odd map
GATE_CASES = [(3, 15, 20, 1152, 48), (2, 1, 1, 32, 8), (2, 30, 40, 144, 6), (1, 120, 160, 96, 4), (2, 7, 3, 240, 1)]
# (B, H, W, Cin, Cout, act, residual, form): every form fpc_mbconv_pw_form can name, each with B >= 2 and H W no multiple of the form's
# tile rows (16 for form 0, 32 for the others), so tiles straddle frames: the widest project site (K = 1152); the 32 x 32 form with one
# channel tile per wave; one row per frame; 2 / 3 / 5 channel tiles per wave (2048 row tiles of 181 x 181 = 32761 rows per frame)
PW_CASES = [(3, 15, 20, 1152, 192, NONE, True, 0), (3, 30, 46, 96, 256, SWISH, False, 1), (3, 1, 1, 8, 8, NONE, True, 0),
            (2, 181, 181, 16, 64, SWISH, False, 2), (2, 181, 181, 24, 96, NONE, True, 3), (2, 181, 181, 8, 160, SWISH, False, 5)]
STEM_CASES = [(1, 2, 2), (2, 6, 10), (1, 64, 96)]


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


def _swish(v):
    return v * torch.sigmoid(v)


def _same_pads(k, s):
    """efficientnet_pytorch's static pads on an even extent, (before, after)."""
    total = k - 1 if s == 1 else k - 2
    return total // 2, total - total // 2


def _dw_ref(x, w, scale, shift, k, s, act):
    C = x.shape[1]
    lo, hi = _same_pads(k, s)
    v = F.conv2d(F.pad(x.double(), (lo, hi, lo, hi)), w.double(), None, s, 0, 1, C)
    v = v * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
    return _swish(v) if act == SWISH else v


def _dw_run(dev, x, w, scale, shift, k, s, act):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, C, Hi, Wi = x.shape
    Ho, Wo = Hi // s, Wi // s
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, sd, hd = w.to(dev), scale.to(dev), shift.to(dev)
    out = _twice(dev, B * Ho * Wo * C, lambda y: L.fpc_mbconv_dw(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y, B, Hi, Wi,
                                                                  C, k, s, act, nat.stream()))
    return out.view(B, Ho, Wo, C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("act", [NONE, SWISH], ids=["plain", "swish"])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("case", DW_CASES, ids=[f"B{b}-{h}x{w}-C{c}" for b, h, w, c in DW_CASES])
def test_depthwise_vs_float64(lib, dev, case, k, s, act):
    B, Hi, Wi, C = case
    g = torch.Generator().manual_seed(1000 * DW_CASES.index(case) + 100 * k + 10 * s + act)
    x = torch.randn((B, C, Hi, Wi), generator=g)
    w = torch.randn((C, 1, k, k), generator=g)
    scale = (torch.rand(C, generator=g) + 0.5) * 2.0
    shift = torch.randn(C, generator=g)
    ref = _dw_ref(x, w, scale, shift, k, s, act)
    assert tuple(ref.shape) == (B, C, Hi // s, Wi // s)
    out = _dw_run(dev, x, w, scale, shift, k, s, act)
    _bar(out, ref, f"mbconv_dw {case} k{k} s{s} act{act}")
    if act == SWISH:
        assert out.min() >= -0.2785                              # swish's minimum
    elif C * Hi * Wi > 64:
        assert out.min() < -1.0


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [3, 5])
def test_depthwise_integer_operands_bit_for_bit(lib, dev, k, s):
    """Small integers: every product and sum is exact in f32, so the output equals float64's whatever the order — and a window that
    starts one cell off (a wrong pad before) cannot hide inside a tolerance."""
    B, Hi, Wi, C = 2, 6, 10, 8
    g = torch.Generator().manual_seed(7 * k + s)
    x = torch.randint(-4, 5, (B, C, Hi, Wi), generator=g).float()
    w = torch.randint(-3, 4, (C, 1, k, k), generator=g).float()
    scale = torch.randint(1, 4, (C,), generator=g).float()
    shift = torch.randint(-5, 6, (C,), generator=g).float()
    ref = _dw_ref(x, w, scale, shift, k, s, NONE)
    other = F.conv2d(x.double(), w.double(), None, s, (k - 1) // 2, 1, C)       # symmetric pads: another result at stride 2
    if s == 2:
        assert not torch.equal(other * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1), ref)
    out = _dw_run(dev, x, w, scale, shift, k, s, NONE)
    assert torch.equal(out.double(), ref)


def _gate_run(dev, x_nhwc, w1, b1, w2, b2):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, H, W, C = x_nhwc.shape
    Cs = w1.shape[0]
    xd, w1d, b1d, w2d, b2d = (t.contiguous().to(dev) for t in (x_nhwc, w1, b1, w2, b2))
    n = L.fpc_mbconv_gate_scratch_floats(B, H, W, C)
    assert n == B * L.fpc_mbconv_gate_slabs(H, W, C) * C > 0
    scratch = torch.full((n + 64,), float("nan"), device=dev)
    out = _twice(dev, B * C, lambda y: L.fpc_mbconv_gate(xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), y,
                                                         scratch.data_ptr(), B, H, W, C, Cs, nat.stream()))
    assert torch.isnan(scratch[n:]).all() and not torch.isnan(scratch[:n]).any()
    return out.view(B, C)


@pytest.mark.parametrize("case", GATE_CASES, ids=[f"B{b}-{h}x{w}-C{c}-Cs{cs}" for b, h, w, c, cs in GATE_CASES])
def test_gate_vs_float64(lib, dev, case):
    from fastposecnn_amd import _native as nat
    B, H, W, C, Cs = case
    g = torch.Generator().manual_seed(300 + GATE_CASES.index(case))
    x = torch.randn((B, H, W, C), generator=g) + torch.randn((1, 1, 1, C), generator=g)      # channel means of order one
    w1 = torch.randn((Cs, C), generator=g) / C ** 0.5
    b1 = torch.randn(Cs, generator=g)
    w2 = torch.randn((C, Cs), generator=g) * 2.0 / Cs ** 0.5
    b2 = torch.randn(C, generator=g)
    mean = x.double().mean(dim=(1, 2))
    ref = torch.sigmoid(_swish(mean @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double())
    assert ref.max() - ref.min() > 0.3
    slabs = nat.lib().fpc_mbconv_gate_slabs(H, W, C)
    assert (slabs > 1) == (case in (GATE_CASES[0], GATE_CASES[2], GATE_CASES[3])), slabs
    _bar(_gate_run(dev, x, w1, b1, w2, b2), ref, f"mbconv_gate {case}")


def test_gate_of_a_constant_plane(lib, dev):
    """x = 2 everywhere on 30 x 40 pixels in two slabs: the mean is exactly 2 (the sum 2400 is exact and the division is IEEE's), the
    reduce with weights 1 / 64 over 32 channels gives exactly 1, the hidden units are swish(1), and the expand with weights 1 / 2 over
    8 units and bias c / 32 gives gate[c] = sigmoid(4 swish(1) + c / 32)."""
    from fastposecnn_amd import _native as nat
    B, H, W, C, Cs = 2, 30, 40, 32, 8
    assert nat.lib().fpc_mbconv_gate_slabs(H, W, C) == 2
    x = torch.full((B, H, W, C), 2.0)
    w1, b1 = torch.full((Cs, C), 1.0 / 64), torch.zeros(Cs)
    w2, b2 = torch.full((C, Cs), 0.5), torch.arange(C).float() / 32
    hid = 1.0 / (1.0 + math.exp(-1.0))
    want = torch.tensor([1.0 / (1.0 + math.exp(-(4.0 * hid + c / 32))) for c in range(C)], dtype=torch.float64)
    out = _gate_run(dev, x, w1, b1, w2, b2)
    assert torch.equal(out[0], out[1])
    # expf's two ulp in swish(1) and the three roundings of the sum of eight reach the gate through sigmoid' < 0.05: under half an
    # ulp of 1; sigmoid's own exp and division add one each
    assert (out[0].double() - want).abs().max().item() <= 4 * 2.0 ** -24


def _pw_run(dev, x, gate, w, scale, shift, res, B, HW, act):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    Cout, Cin = w.shape[:2]
    p = lambda t: None if t is None else t.data_ptr()
    return _twice(dev, B * HW * Cout, lambda y: L.fpc_mbconv_pw(p(x), p(gate), p(w), p(scale), p(shift), p(res), y, B, HW, Cin, Cout, act,
                                                                nat.stream())).view(B * HW, Cout)


@pytest.mark.parametrize("case", PW_CASES, ids=[f"B{b}-{h}x{w}-{ci}to{co}-act{a}-res{int(r)}-form{f}" for b, h, w, ci, co, a, r, f in PW_CASES])
def test_gated_1x1_vs_float64(lib, dev, case):
    from fastposecnn_amd import _native as nat
    B, H, W, Cin, Cout, act, has_res, form = case
    HW, M = H * W, B * H * W
    assert nat.lib().fpc_mbconv_pw_form(B, HW, Cin, Cout) == form
    assert HW % (16 if form == 0 else 32) != 0 and B >= 2
    g = torch.Generator().manual_seed(400 + PW_CASES.index(case))
    x = torch.randn((M, Cin), generator=g)
    gate = torch.sigmoid(torch.randn((B, Cin), generator=g) * 2.0)
    w = torch.randn((Cout, Cin, 1, 1), generator=g) * 2.0 / Cin ** 0.5
    scale = (torch.rand(Cout, generator=g) + 0.5) * 2.0
    shift = torch.randn(Cout, generator=g)
    res = torch.randn((M, Cout), generator=g)
    w64 = w.double().view(Cout, Cin).t()

    def ref_of(xg):
        v = xg @ w64 * scale.double() + shift.double()
        return _swish(v) if act == SWISH else v
    gated = x.double().view(B, HW, Cin) * gate.double().view(B, 1, Cin)
    ref, ref_plain = ref_of(gated.view(M, Cin)), ref_of(x.double())
    assert (ref - ref_plain).abs().max() > 0.1                   # the gate matters, frame by frame
    xd, gd, wd, sd, hd, rd = (t.to(dev) for t in (x, gate, w, scale, shift, res))
    out = _pw_run(dev, xd, gd, wd, sd, hd, None, B, HW, act)
    _bar(out, ref, f"mbconv_pw {case}")
    for b in range(B):                                           # (each frame against its own gate: a tile's rows of two frames)
        _bar(out[b * HW:(b + 1) * HW], ref[b * HW:(b + 1) * HW], f"mbconv_pw {case} frame {b}")
    if act == SWISH:
        assert out.min() >= -0.2785 and (out < 0).any()
    plain = _pw_run(dev, xd, None, wd, sd, hd, None, B, HW, act)
    _bar(plain, ref_plain, f"mbconv_pw {case} without gate")
    ones = _pw_run(dev, xd, torch.ones_like(gd), wd, sd, hd, None, B, HW, act)
    assert torch.equal(ones, plain)                              # gate NULL and gate = 1: the same bits
    if has_res:
        with_res = _pw_run(dev, xd, gd, wd, sd, hd, rd, B, HW, act)
        _bar(with_res, ref + res.double(), f"mbconv_pw {case} + res")
        assert not torch.equal(with_res, out)


@pytest.mark.parametrize("case", PW_CASES, ids=[f"B{b}-{h}x{w}-{ci}to{co}-form{f}" for b, h, w, ci, co, a, r, f in PW_CASES])
def test_gated_1x1_integer_operands_bit_for_bit(lib, dev, case):
    """Small integers and gates that are powers of two, another per frame: every product in . gate, every product with w and every
    partial sum is exact in f32 (|sum| <= 1152 x 8 x 2 in steps of 1 / 4), so the output equals float64's bit for bit, act none."""
    B, H, W, Cin, Cout, _, _, _ = case
    HW, M = H * W, B * H * W
    g = torch.Generator().manual_seed(500 + PW_CASES.index(case))
    x = torch.randint(-4, 5, (M, Cin), generator=g).float()
    gate = 2.0 ** torch.randint(-2, 2, (B, Cin), generator=g).float()
    w = torch.randint(-2, 3, (Cout, Cin, 1, 1), generator=g).float()
    scale = torch.randint(1, 4, (Cout,), generator=g).float()
    shift = torch.randint(-5, 6, (Cout,), generator=g).float()
    res = torch.randint(-9, 10, (M, Cout), generator=g).float()
    gated = (x.double().view(B, HW, Cin) * gate.double().view(B, 1, Cin)).view(M, Cin)
    ref = gated @ w.double().view(Cout, Cin).t() * scale.double() + shift.double() + res.double()
    xd, gd, wd, sd, hd, rd = (t.to(dev) for t in (x, gate, w, scale, shift, res))
    out = _pw_run(dev, xd, gd, wd, sd, hd, rd, B, HW, NONE)
    assert torch.equal(out.double(), ref)


@pytest.mark.parametrize("B,Hi,Wi", STEM_CASES)
def test_stem_vs_float64(lib, dev, B, Hi, Wi):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    g = torch.Generator().manual_seed(1000 + Hi * 100 + Wi)
    x = torch.randn((B, 3, Hi, Wi), generator=g)
    w = torch.randn((32, 3, 3, 3), generator=g) / 27 ** 0.5
    scale = (torch.rand(32, generator=g) + 0.5) * 4.0
    shift = torch.randn(32, generator=g)
    ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), None, 2, 0) * scale.double().view(1, 32, 1, 1) + shift.double().view(1, 32, 1, 1)
    ref = _swish(ref)
    Ho, Wo = Hi // 2, Wi // 2
    assert tuple(ref.shape) == (B, 32, Ho, Wo)
    x4 = torch.full((B, Hi, Wi, 4), float("nan"), device=dev)
    assert L.fpc_image_nhwc4(x.to(dev).data_ptr(), x4.data_ptr(), B, Hi, Wi, nat.stream()) == 0
    wd, sd, hd = w.to(dev), scale.to(dev), shift.to(dev)
    out = _twice(dev, ref.numel(), lambda y: L.fpc_mbconv_stem(x4.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y, B, Hi, Wi, 32,
                                                               nat.stream()))
    out = out.view(B, Ho, Wo, 32).permute(0, 3, 1, 2)
    _bar(out, ref, f"mbconv_stem {(B, Hi, Wi)}")
    assert out.min() >= -0.2785
    if Hi > 2:
        assert (out < 0).any() and out.max() > 2.0


def _model(lib, seed=0):
    """test_gpu_mobilenet_v2.py's model on efficientnet-b0: random BatchNorm and GroupNorm statistics and affines."""
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = ENCODER
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
    for name, f, C in zip(("c2", "c3", "c4", "c5"), feats[2:], (24, 40, 112, 320)):
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
    assert len(plans) == 44 and [p[4] for p in plans[:4]] == [320, 112, 40, 24]          # the decoders' sites alone
    if split == "f32":
        assert not any(p[2] >= 1000 for p in plans)                                      # level 0: f32 products only
    with pytest.raises(RuntimeError):
        eng.force_stem_pool(1)
    with pytest.raises(RuntimeError):
        eng.force_fold(1)
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
    print("efficientnet-b0 B=1 plans:", eng.conv_plans())


# The bias of a project BatchNorm (_bn2) shifts its block's output by a constant per channel.  That constant rides through the skip adds
# of the blocks behind it and dies at the first expand 1x1 followed by a training-mode BatchNorm (which removes a per-channel constant
# exactly; every block behind block 0 has one, and a 1x1 reads no padding).  So the bias has a gradient only where skip adds alone carry
# it to a tapped feature level (blocks 2, 4, 8 and 15, read by the laterals): blocks 1-2, 3-4, 8 and 15.  For blocks 0, 5-7 and 9-14
# it has NONE: float64 returns 1e-17 there and f32 its rounding noise, and "relative to the parameter's own gradient" would compare
# noise with noise.  Derived from the module's skip flags and smp's stage ends, not from a run.
def _zero_grad_biases(encoder):
    taps = {s - 1 for s in encoder._stage_idxs}
    n = len(encoder._blocks)
    out = set()
    for i in range(n):
        j, alive = i, i in taps
        while not alive and j + 1 < n and encoder._blocks[j + 1].use_skip:
            j += 1
            alive = j in taps
        if not alive:
            out.add(f"encoder._blocks.{i}._bn2.bias")
    return out


def test_training_step_native_vs_torch(lib, dev, monkeypatch):
    """Forward + backward of a small efficientnet-b0 model in training mode with drop-connect off: the native convolutions and
    BatchNorms against the same model on torch's f32 kernels, each against float64 — test_gpu_mobilenet_v2.py's form and bars.  The
    decoders' ReLU is swapped for Softplus (its kink at 0 would make f32 and float64 gradients disagree arbitrarily; swish is smooth
    and stays); the depthwise convolutions, swish, the pooling and the sigmoid multiply are torch's on both sides."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = ENCODER
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    assert model.encoder.drop_connect_rate == 0.2
    model.encoder.drop_connect_rate = 0.0
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
        for name, child in list(mod.named_children()):
            if isinstance(child, (torch.nn.ReLU, torch.nn.ReLU6)):
                setattr(mod, name, torch.nn.Softplus())
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
    print("efficientnet-b0 training step: counters", used)
    assert used["fwd_native"] > 0, used                # the dense sites the front end accepts
    assert unused["fwd_native"] == 0
    assert abs(ln - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in orf:
        assert (on[k] - orf[k]).abs().max().item() <= 1e-4 * max(1.0, orf[k].abs().max().item()), k
    # every parameter the forward runs has a gradient; _conv_head and the top-level _bn1 are not run and have none
    idle = {"encoder._conv_head.weight", "encoder._bn1.weight", "encoder._bn1.bias"}
    names = [n for n, p in model.named_parameters() if p.requires_grad and n not in idle]
    assert set(gn) == set(gr) == set(names), "a parameter without a gradient"
    # the stem, 15 expand, 16 depthwise and 16 project convolutions with their BatchNorms' weight and bias, and 16 gates of four
    assert sum(n.startswith("encoder.") for n in names) == 3 * 48 + 4 * 16
    assert "encoder._blocks.0._se_reduce.bias" in gn and "encoder._blocks.15._project_conv.weight" in gn
    err_n = err_t = 0.0
    worst = None
    ZERO_GRAD = _zero_grad_biases(model.encoder)
    assert sorted(int(n.split(".")[2]) for n in ZERO_GRAD) == [0, 5, 6, 7, 9, 10, 11, 12, 13, 14]
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
    print("efficientnet-b0 training step: err native", err_n, "torch", err_t, "worst", worst)
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)
