"""Models of 9 to 32 classes on the native backbone engine: the sliced merge + head passes (k_head_part_wide, heads of 33 to 128
channels) and the four-pixel x4 upsample + class compression (k_up4_compress_wide), against float64.

All models are resnet18 with random weights and non-trivial BatchNorm / GroupNorm parameters (the `_model` recipe of
test_gpu_net.py), ENGINE_AUTOTUNE = False (static plans: built in well under a second, the same bits on every build).

The <= 8-class routes (k_head_part<*, *>, k_up4_compress7x4 / 7 / <8>, k_merge_head) have no new switch: their kernels, their
launch conditions and their plans are not touched, and the existing suite (test_plan_contract.py, test_gpu_net.py) holds them.
"""
import copy
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

# ---- the bar of the localised x4 upsample + compression test (test 3).  Error measure: max |got - ref| / max(1, max |ref|) per
# tensor, ref = float64 bilinear (align_corners) x4 interpolation of the engine's own low-resolution tensors.  The existing 7-class
# route (k_up4_compress7x4) on the same harness (same recipe, same mask-head shaping, the three shapes of UP4_SHAPES) attains
# 2.75e-7 / 8.43e-7 / 7.66e-7 at 3x32x32 / 1x32x96 / 2x64x128 (the mask head each time; the source coordinates are f32 in the
# kernels and f64 in the reference, so the figure grows with the map's size): UP4_MEASURED_7 is the worst of them.  The new form is
# held to twice that, 1.688e-6 (the margin covers a different but equally valid association of the same four-tap sum); it attains
# 3.8e-7 / 7.2e-7 / 8.4e-7 at 10 classes and 3.1e-7 / 5.1e-7 / 8.8e-7 at 32.
UP4_MEASURED_7 = 8.44e-7
UP4_BAR = 2 * UP4_MEASURED_7

ENGINE_CASES = [(9, 3, 32, 32), (10, 3, 32, 32), (17, 3, 32, 32), (18, 3, 32, 32), (26, 3, 32, 32), (32, 3, 32, 32),
                (10, 1, 32, 96), (32, 1, 32, 96), (10, 2, 64, 128), (32, 2, 64, 128)]
UP4_SHAPES = [(3, 32, 32), (1, 32, 96), (2, 64, 128)]
UP4_CASES = [(c,) + s for c in (10, 32) for s in UP4_SHAPES]
UP4_SEED = {(3, 32, 32): 2, (1, 32, 96): 5, (2, 64, 128): 2}      # per shape: every label of 10 and of 32 classes wins somewhere

DECODERS = (("mask_decoder", "segmentation_head"), ("rotation_decoder", "rotation_head"),
            ("translation_decoder", "translation_head"), ("scales_decoder", "scales_head"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fastposecnn_amd import _native
    _native.lib()
    return torch.device("cuda:0")


def _model(classes, seed=0):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet18"
    hp.PERFORM_AGGREGATION = False
    hp.ENGINE_AUTOTUNE = False
    hp.SELECTED_CLASSES = ["bg"] + ["obj%d" % i for i in range(1, classes)]
    torch.manual_seed(seed)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
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
    assert m.classes == classes
    return m.eval(), hp


def _images(B, H, W):
    from fastposecnn_amd import synth
    return torch.stack([synth.make_image(i, H, W) for i in range(B)])


def _double(m, hp):
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp)
    ref_m.HPARAM.USE_NATIVE_ENGINE = False
    return ref_m


def _low64(ref_m, x64):
    """(encoder features, the four heads' logits at 1/4 resolution: decoder + 1x1 head, no x4 upsample), float64."""
    with torch.no_grad():
        feats = ref_m.encoder(x64)
        low = [getattr(ref_m, head)[0](getattr(ref_m, dec)(*feats)) for dec, head in DECODERS]
    return feats, low


def _up4_64(low):
    """float64 x4 bilinear (align_corners) upsample of NCHW low-resolution logits [mask, quat, xyz, scales] -> the logits dict."""
    up = [F.interpolate(t, scale_factor=4, mode="bilinear", align_corners=True) for t in low]
    n = up[2].shape[1] // 3
    xy = [3 * k + e for k in range(n) for e in (0, 1)]
    z = [3 * k + 2 for k in range(n)]
    return {"mask": up[0], "quaternion": up[1], "scales": up[3], "xy": up[2][:, xy], "z": up[2][:, z]}


def _rel(got, ref):
    return (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------------------------
# tests 1 + 2: the engine against the float64 module path, whole and at the head stage

@functools.lru_cache(maxsize=None)
def _engine_run(classes, B, H, W):
    dev = torch.device("cuda:0")
    m, hp = _model(classes)
    x = _images(B, H, W)
    ref_m = _double(m, hp)
    feats, low = _low64(ref_m, x.double())
    with torch.no_grad():
        ref = ref_m.pure_model_forward(x.double())
    m = m.to(dev)
    with torch.no_grad():
        out = m(x.to(dev))
    assert m._engines, "the native engine did not run"
    eng = next(iter(m._engines.values()))
    got_feats = [eng.tensor(n).permute(0, 3, 1, 2).cpu().double() for n in ("c2", "c3", "c4", "c5")]
    got_low = [eng.tensor("d%d.low" % d).cpu().double() for d in range(4)]      # NHWC, chp channels
    got = {k: v.cpu().double() for k, v in out["logits"].items()}
    return dict(feats=feats[2:], got_feats=got_feats, low=low, got_low=got_low, ref=ref, got=got)


@gpu
@pytest.mark.parametrize("classes,B,H,W", ENGINE_CASES)
def test_engine_vs_float64(dev, classes, B, H, W):
    """c2 .. c5 and the five logit tensors within 1e-4 max(1, |ref|max) of the float64 module path (test_net_vs_float64_cpu's bar)."""
    r = _engine_run(classes, B, H, W)
    for name, got, f in zip(("c2", "c3", "c4", "c5"), r["got_feats"], r["feats"]):
        err = (got - f).abs().max().item()
        assert err <= 1e-4 * max(1.0, f.abs().max().item()), (name, err)
    G = classes - 1
    for k, ch in (("mask", classes), ("quaternion", 4 * G), ("scales", 3 * G), ("xy", 2 * G), ("z", G)):
        got, ref = r["got"][k], r["ref"][k]
        assert got.shape == ref.shape == (B, ch, H, W), k
        err = (got - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (k, err)


@gpu
@pytest.mark.parametrize("classes,B,H,W", ENGINE_CASES)
def test_head_stage_vs_float64(dev, classes, B, H, W):
    """The two head passes alone: d<k>.low[..., :ch] against the float64 decoder + head at 1/4 resolution (no x4 upsample), the same
    bar; the padding channels ch .. chp are finite (the passes write zeros there)."""
    r = _engine_run(classes, B, H, W)
    G = classes - 1
    for d, ch in enumerate((classes, 4 * G, 3 * G, 3 * G)):
        got, ref = r["got_low"][d], r["low"][d].permute(0, 2, 3, 1)
        assert got.shape == (B, H // 4, W // 4, (ch + 3) // 4 * 4), d
        err = (got[..., :ch] - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (d, err)
        assert torch.isfinite(got[..., ch:]).all(), d


# ------------------------------------------------------------------------------------------------------------------------------
# test 3: the x4 upsample + class compression alone

def _shaped_model(classes, B, H, W):
    """The recipe's model with a mask head whose classes all win somewhere at clear margins: every class's weight row and bias
    scaled and its bias moved so that its low-resolution logit has mean 0 and standard deviation 8 over the test input (float64,
    on the CPU)."""
    m, hp = _model(classes, seed=UP4_SEED[(B, H, W)])
    x = _images(B, H, W)
    conv = m.segmentation_head[0]
    with torch.no_grad():
        _, low = _low64(_double(m, hp), x.double())
        s = (8.0 / low[0].std(dim=(0, 2, 3))).float()
        mu = low[0].mean(dim=(0, 2, 3)).float()
        conv.weight.mul_(s[:, None, None, None])
        conv.bias.copy_((conv.bias - mu) * s)
    return m, hp, x


def _label_margins(mask64):
    """(arg-max labels, top-two gap) of float64 mask logits [B, C, H, W]."""
    top = mask64.topk(2, dim=1)
    return top.indices[:, 0], top.values[:, 0] - top.values[:, 1]


@pytest.mark.parametrize("classes,B,H,W", UP4_CASES)
def test_up4_reference_has_clear_labels_of_every_class(classes, B, H, W):
    """Properties of the float64 reference alone (CPU): on the shaped model fewer than 0.5 % of each frame's pixels have a top-two
    gap under the bar, and every one of the `classes` labels wins somewhere."""
    m, hp, x = _shaped_model(classes, B, H, W)
    _, low = _low64(_double(m, hp), x.double())
    mask = _up4_64(low)["mask"]
    labels, gap = _label_margins(mask)
    bar = UP4_BAR * max(1.0, mask.abs().max().item())
    share = (gap < bar).double().mean(dim=(1, 2))
    assert share.max().item() < 0.005, share
    assert sorted(labels.unique().tolist()) == list(range(classes))


@functools.lru_cache(maxsize=None)
def _up4_run(classes, B, H, W):
    dev = torch.device("cuda:0")
    m, hp, x = _shaped_model(classes, B, H, W)
    m = m.to(dev)
    with torch.no_grad():
        m(x.to(dev))
        eng = next(iter(m._engines.values()))
        logits, cat = eng.forward(x.to(dev))
    G = classes - 1
    low = [eng.tensor("d%d.low" % d).cpu().double()[..., :ch].permute(0, 3, 1, 2).contiguous()
           for d, ch in enumerate((classes, 4 * G, 3 * G, 3 * G))]
    ref = _up4_64(low)
    bits = getattr(cat["mask"], "_fpc_fg_bits", None)
    return dict(ref=ref, got={k: v.cpu().double() for k, v in logits.items()}, cat={k: v.cpu() for k, v in cat.items()},
                bits=None if bits is None else bits[0].cpu())


def _check_up4(r, classes, B, H, W, bar_rel):
    ref, got, cat = r["ref"], r["got"], r["cat"]
    errs = {k: _rel(got[k], ref[k]) for k in ref}
    print("up4 logits error (max |d| / max(1, |ref|max)) at %d classes %dx%dx%d:" % (classes, B, H, W), errs)
    assert max(errs.values()) <= bar_rel, errs
    labels, gap = _label_margins(ref["mask"])
    sure = gap >= bar_rel * max(1.0, ref["mask"].abs().max().item())
    assert (~sure).double().mean(dim=(1, 2)).max().item() <= 0.01
    assert torch.equal(cat["mask"][sure], labels[sure])
    assert int(cat["mask"].min()) >= 0 and int(cat["mask"].max()) < classes
    agree = cat["mask"] == labels
    g = (labels - 1).clamp(min=0)
    fg = (labels > 0).double()

    def pick(t, n):      # channels n g .. n g + n - 1 of every pixel's own class, zeros on the background
        idx = (n * g)[:, None] + torch.arange(n)[None, :, None, None]
        return t.gather(1, idx) * fg[:, None]
    q, sc = pick(ref["quaternion"], 4), pick(ref["scales"], 3)
    xy, z = pick(ref["xy"], 2), pick(ref["z"], 1)[:, 0]
    # quaternion and xy leave the kernel divided by their norm, which magnifies the interpolation error of a short vector by
    # 1 / norm (xy norms of 0.05 occur): they are compared in the logits' own units, kernel output x the reference's norm against
    # the reference's selected values, so that the bar stays the logits bar of that head; that the output is a unit vector (or
    # zero) is checked apart, to 1e-6 (four products, three additions, a root and a division in f32: under 8 ulp of 1)
    nq = q.norm(dim=1, keepdim=True)
    nv = xy.norm(dim=1, keepdim=True)
    for k, want, scale, head in (("quaternion", q, nq, "quaternion"), ("scales", sc, None, "scales"), ("xy", xy, nv, "xy"),
                                 ("z", z, None, "z")):
        got_k = cat[k].double()
        a = agree if want.dim() == 3 else agree[:, None].expand_as(want)
        if scale is not None:
            unit = got_k.norm(dim=1, keepdim=True)
            ok = ((unit - 1).abs() <= 1e-6) | ((unit == 0) & (scale == 0))
            assert ok[agree[:, None]].all(), k
            got_k = got_k * scale
        d = ((got_k - want).abs() * a).max().item()
        print("  selected %s: %.3g" % (k, d / max(1.0, ref[head].abs().max().item())))
        assert d <= bar_rel * max(1.0, ref[head].abs().max().item()), (k, d)
    if r["bits"] is not None:      # the foreground bit plane: cat_mask != 0 packed 64 pixels to a word, exactly
        words = ((cat["mask"] != 0).view(B, H * W // 64, 64).long() << torch.arange(64)).sum(-1)
        assert torch.equal(r["bits"][:, :H * W // 64], words)
    return errs


@gpu
def test_up4_seven_class_route_sets_the_bar(dev):
    """The measurement behind UP4_BAR: the existing 7-class route (k_up4_compress7x4) on this harness attains UP4_MEASURED_7 against
    the float64 interpolation of its own low-resolution tensors; it must itself pass the checks the new form is held to."""
    worst = 0.0
    for B, H, W in UP4_SHAPES:
        errs = _check_up4(_up4_run(7, B, H, W), 7, B, H, W, UP4_BAR)
        worst = max(worst, max(errs.values()))
    print("7-class route, worst logits error:", worst, "(UP4_MEASURED_7 = %g)" % UP4_MEASURED_7)
    assert worst <= UP4_MEASURED_7 * 1.0001


@gpu
@pytest.mark.parametrize("classes,B,H,W", UP4_CASES)
def test_up4_wide_vs_float64(dev, classes, B, H, W):
    """k_up4_compress_wide against float64 computed from the engine's own d<k>.low: logits within UP4_BAR = 1.688e-6 (twice the
    8.44e-7 the 7-class route attains; measured for this form: at most 8.8e-7); labels equal to the reference's arg-max wherever its top-two gap is at least the bar (at most 1 %
    of a frame is left out); where the labels agree, the selected and normalised planes within the bar; the bit words exact."""
    _check_up4(_up4_run(classes, B, H, W), classes, B, H, W, UP4_BAR)


# ------------------------------------------------------------------------------------------------------------------------------
# test 4: modes and replay, bit for bit

def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("classes", [10, 32])
def test_modes_and_replay_are_bit_identical(dev, classes, monkeypatch):
    from fastposecnn_amd.streaming import FrameStreamer
    B, H, W = 2, 64, 128
    m, hp = _model(classes)
    m = m.to(dev)
    hp.ENGINE_GRAPH = False
    x = _images(B, H, W).to(dev)
    with torch.no_grad():
        logits = m.pure_model_forward(x)
        cat = m.class_compression(logits)
        eng = next(iter(m._engines.values()))
        l1, c1 = eng.forward(x)                                   # a second forward of the same plan
        none, c0 = eng.forward(x, want_logits=False)             # the streaming mode: no logit planes
        torch.cuda.synchronize()
        assert none is None
        _same(logits, l1)
        _same(cat, c1)
        _same(cat, c0)
        b1, b0 = getattr(c1["mask"], "_fpc_fg_bits", None), getattr(c0["mask"], "_fpc_fg_bits", None)
        assert (b1 is None) == (b0 is None)
        if b1 is not None:
            assert torch.equal(b1[0][:, :H * W // 64], b0[0][:, :H * W // 64])
        # the range guard's surveying forward (it may move sites of this random model off the fp16-piece forms, for good: the
        # plan it leaves gives the surveyed frame's bits again, and the outputs stay at the float64 bar of the earlier ones)
        hp.ENGINE_RANGE_GUARD = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            lg = m.pure_model_forward(x)
        cg = m.class_compression(lg)
        hp.ENGINE_RANGE_GUARD = False
        lg2 = m.pure_model_forward(x)
        cg2 = m.class_compression(lg2)
        _same(lg, lg2)
        _same(cg, cg2)
        for k in logits:
            assert (lg[k] - logits[k]).abs().max().item() <= 2e-4 * max(1.0, logits[k].abs().max().item()), k
        # the generic one-pixel kernel on the same plan (FPC_UP4_WIDE=0 is read when a plan is created)
        monkeypatch.setenv("FPC_UP4_WIDE", "0")
        m._drop_engines()
        lo = m.pure_model_forward(x)
        co = m.class_compression(lo)
        monkeypatch.delenv("FPC_UP4_WIDE")
        _same(logits, lo)
        _same(cat, co)
        # graph replay on a side stream against the plain launches
        hp.ENGINE_GRAPH = True
        m._drop_engines()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                lr = m.pure_model_forward(x)
                cr = m.class_compression(lr)
        side.synchronize()
        assert next(iter(m._engines.values())).graph_recorded()
        _same(logits, lr)
        _same(cat, cr)
        # a FrameStreamer frame (its own plan copies, its own streams, graphs) against forward
        st = FrameStreamer(m, net_streams=2)
        st.prepare(x)
        outs = [st.collect(t) for t in [st.submit(x) for _ in range(3)]]
    for o in outs:
        _same(logits, o["logits"])
        _same(cat, o["categorical"])


# ------------------------------------------------------------------------------------------------------------------------------
# test 5: the whole forward at 12 classes

@gpu
def test_whole_forward_at_12_classes(dev):
    """m(x) with aggregation, hough voting and RT calculation on: the reference's dict schema, class ids in 1 .. 11, finite poses."""
    m, hp = _model(12)
    hp.PERFORM_AGGREGATION = True
    hp.PERFORM_HOUGH_VOTING = True
    hp.PERFORM_RT_CALCULATION = True
    hp.HV_NUM_OF_HYPOTHESES = 32
    m = m.to(dev)
    B, H, W = 2, 64, 96
    x = _images(B, H, W).to(dev)
    with torch.no_grad():
        torch.manual_seed(5)
        out = m(x)
    assert m._engines, "the native engine did not run"
    assert set(out) == {"logits", "categorical", "aggregated"}
    assert tuple(out["logits"]["quaternion"].shape) == (B, 44, H, W) and tuple(out["logits"]["mask"].shape) == (B, 12, H, W)
    assert int(out["categorical"]["mask"].min()) >= 0 and int(out["categorical"]["mask"].max()) <= 11
    agg = out["aggregated"]
    n = agg["class_ids"].shape[0]
    print("instances found at 12 classes:", n)
    for k, shp in (("instance_masks", (n, H, W)), ("quaternion", (n, 4)), ("scales", (n, 3)), ("xy", (n, 2)),
                   ("z", (n, 1)), ("R", (n, 3, 3)), ("T", (n, 3)), ("RT", (n, 4, 4)), ("hypothesis", (n, 1, 2)),
                   ("xy_mask", (n, 2, H, W)), ("sample_ids", (n,))):
        assert tuple(agg[k].shape) == shp, k
    assert n > 0
    assert int(agg["class_ids"].min()) >= 1 and int(agg["class_ids"].max()) <= 11 and int(agg["sample_ids"].max()) <= B - 1
    for k in ("R", "T", "RT"):
        assert torch.isfinite(agg[k]).all(), k
