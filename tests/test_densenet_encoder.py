"""CPU checks of the DenseNet encoders (densenet121 / 169 / 201): the module restatement against the published definition of
torchvision's DenseNet as smp's DenseNetEncoder wraps it (parameter counts by plain arithmetic, state-dict names against committed
manifests, feature levels, BatchNorm constants, a dense layer and a transition against formulas in float64, the transition's two
orders), encoder-weights loading with the legacy keys, the preprocessing parameters, the engine's host-side plan
(fpc_net_create("densenet121" ...): parameter table, refusals), the host-side refusals of the stand-alone kernel entries, and the
condition the GPU engine test puts on its own inputs.  No compute calls into the HIP library."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import _batch_forms as BF
import _densenet_model as D

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS = {"densenet121": (6, 12, 24, 16), "densenet169": (6, 12, 32, 32), "densenet201": (6, 12, 48, 32)}
PARAMS = {"densenet121": 6_953_856, "densenet169": 12_484_480, "densenet201": 18_092_928}
KEYS = {"densenet121": 725, "densenet169": 1013, "densenet201": 1205}
OUT = {"densenet121": (3, 64, 256, 512, 1024, 1024), "densenet169": (3, 64, 256, 512, 1280, 1664),
       "densenet201": (3, 64, 256, 512, 1792, 1920)}
NAMES = sorted(BLOCKS)


def params_by_arithmetic(name):
    """Weights and BatchNorm affines: stem 64, growth 32, bn_size 4, a transition halves the channels."""
    total = 64 * 3 * 49 + 2 * 64
    c = 64
    for b, layers in enumerate(BLOCKS[name]):
        for _ in range(layers):
            total += 2 * c + 128 * c + 2 * 128 + 32 * 128 * 9
            c += 32
        if b < 3:
            total += 2 * c + (c // 2) * c
            c //= 2
    return total + 2 * c


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


@pytest.fixture(scope="module")
def encs():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(0)
    return {n: bb.get_encoder(n) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_parameter_counts(encs, name):
    assert params_by_arithmetic(name) == PARAMS[name]
    assert sum(p.numel() for p in encs[name].parameters()) == PARAMS[name]


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_key_order_equals_the_manifest(encs, name):
    """The manifests are written by tests/golden/make_state_dict_keys_densenet.py from the published definition, not dumped from this
    module."""
    want = open(os.path.join(HERE, "golden", f"state_dict_keys_{name}.txt")).read().split()
    assert len(want) == KEYS[name]
    sd = encs[name].state_dict()
    assert list(sd) == want
    assert not any(k.startswith("classifier") or k.endswith(".bias") and ".conv" in k for k in want)
    assert want[0] == "features.conv0.weight" and want[-1] == "features.norm5.num_batches_tracked"
    assert tuple(sd["features.conv0.weight"].shape) == (64, 3, 7, 7)
    last = BLOCKS[name][3]
    assert tuple(sd[f"features.denseblock4.denselayer{last}.conv1.weight"].shape) == (128, OUT[name][5] - 32, 1, 1)
    assert tuple(sd[f"features.denseblock4.denselayer{last}.conv2.weight"].shape) == (32, 128, 3, 3)
    assert tuple(sd["features.transition3.conv.weight"].shape) == (OUT[name][4] // 2, OUT[name][4], 1, 1)


@pytest.mark.parametrize("name", NAMES)
def test_module_properties(encs, name):
    from fastposecnn_amd.lib import backbone as bb
    enc = encs[name]
    assert isinstance(enc, bb.DenseNetEncoder) and enc.name == name and enc.out_channels == OUT[name]
    assert bb.encoder_family(name) == "densenet" and bb.encoder_family("resnet18") == "resnet"
    assert name in bb._available()
    assert not hasattr(enc, "classifier") and not hasattr(enc.features, "classifier")
    torch.manual_seed(1)
    with torch.no_grad():
        feats = enc.eval()(torch.randn(1, 3, 64, 96))
    c = OUT[name]
    assert [tuple(f.shape[1:]) for f in feats] == [(3, 64, 96), (64, 32, 48), (c[2], 16, 24), (c[3], 8, 12), (c[4], 4, 6), (c[5], 2, 3)]
    assert all(torch.isfinite(f).all() for f in feats)
    assert all(f.min() >= 0 for f in feats[1:5]) and feats[5].min() < 0      # levels 1 .. 4 lie behind a ReLU, level 5 is norm5's output
    bns = [m for m in enc.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 1 + 2 * sum(BLOCKS[name]) + 3 + 1
    assert all(isinstance(m, bb.BatchNorm2d) and m.eps == 1e-5 and m.momentum == 0.1 for m in bns)
    convs = [m for m in enc.modules() if isinstance(m, torch.nn.Conv2d)]
    assert all(isinstance(m, bb.Conv2d) and m.bias is None for m in convs)
    assert isinstance(enc.features.pool0, bb.MaxPool2d) and enc.features.pool0.kernel_size == 3 and enc.features.pool0.padding == 1
    relus = [n for n, m in enc.named_modules() if isinstance(m, torch.nn.ReLU)]
    assert len(relus) == 1 + 2 * sum(BLOCKS[name]) + 3                       # every ReLU is a named child module


def test_densenet161_and_other_names_are_refused():
    from fastposecnn_amd.lib import backbone as bb
    for other in ("densenet161", "densenet", "densenet-121", "densenet264"):
        with pytest.raises(KeyError):
            bb.encoder_family(other)
        with pytest.raises(KeyError, match="densenet121"):      # the message lists what there is
            bb.get_encoder(other)
    assert "densenet161" not in bb._available()


def _bn64(x, bn):
    v = lambda t: t.double().view(1, -1, 1, 1)
    return (x - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + 1e-5) * v(bn.weight) + v(bn.bias)


def _randomise(mod, g):
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.3)


def test_dense_layer_and_transition_against_the_formula():
    from fastposecnn_amd.lib import backbone as bb
    g = torch.Generator().manual_seed(3)
    torch.manual_seed(3)
    layer = bb.DenseLayer(96, 32, 4).double().eval()
    block = bb.DenseBlock(2, 64, 32, 4).double().eval()
    tr = bb.Transition(128, 64).double().eval()
    for m in (layer, block, tr):
        _randomise(m, g)
    x = torch.randn((2, 96, 5, 7), generator=g, dtype=torch.float64)
    with torch.no_grad():
        y = layer(x.clone())
        want = F.conv2d(_bn64(F.conv2d(_bn64(x, layer.norm1).clamp_min(0), layer.conv1.weight), layer.norm2).clamp_min(0), layer.conv2.weight,
                        None, 1, 1)
        assert tuple(y.shape) == (2, 32, 5, 7) and torch.allclose(y, want, rtol=0, atol=1e-12)
        # a block: the layers' outputs behind the input, in order
        xb = x[:, :64].contiguous()
        yb = block(xb.clone())
        l1 = block["denselayer1"](xb.clone())
        l2 = block["denselayer2"](torch.cat([xb, l1], 1))
        assert tuple(yb.shape) == (2, 128, 5, 7) and torch.equal(yb, torch.cat([xb, l1, l2], 1))
        # a transition: the skip tensor is relu(norm(x)), the output the 2 x 2 mean of its 1x1 convolution
        xt = torch.randn((2, 128, 6, 8), generator=g, dtype=torch.float64)
        pooled, skip = tr(xt.clone())
        s = _bn64(xt, tr.norm).clamp_min(0)
        c = F.conv2d(s, tr.conv.weight)
        want = 0.25 * (c[:, :, 0::2, 0::2] + c[:, :, 0::2, 1::2] + c[:, :, 1::2, 0::2] + c[:, :, 1::2, 1::2])
        assert torch.allclose(skip, s, rtol=0, atol=1e-12) and torch.allclose(pooled, want, rtol=0, atol=1e-12)
        # the engine's order, conv(pool(.)): the same linear map
        other = F.conv2d(F.avg_pool2d(skip, 2, 2), tr.conv.weight)
        assert (other - pooled).abs().max().item() <= 1e-12 * pooled.abs().max().item()


def test_encoder_weights_file_with_legacy_keys_and_classifier(tmp_path, monkeypatch):
    import re
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(4)
    donor = bb.DenseNetEncoder("densenet121")
    sd = donor.state_dict()
    legacy = {}
    for k, v in sd.items():      # torchvision's released files: denselayerN.norm.1.weight, .conv.2.weight ...
        legacy[re.sub(r"(denselayer\d+\.(?:norm|conv))([12])\.", r"\1.\2.", k)] = v.clone()
    assert "features.denseblock1.denselayer1.norm.1.weight" in legacy and "features.denseblock4.denselayer16.conv.2.weight" in legacy
    assert "features.transition1.norm.weight" in legacy and "features.norm5.weight" in legacy and len(legacy) == len(sd)
    assert sum(k in sd for k in legacy) == 6 + 3 * 6 + 5      # only the stem, the transitions and norm5 keep their names
    legacy["classifier.weight"] = torch.zeros(1000, 1024); legacy["classifier.bias"] = torch.zeros(1000)
    f = tmp_path / "densenet121.pth"
    torch.save(legacy, f)
    monkeypatch.setenv("FPC_ENCODER_WEIGHTS", str(f))
    torch.manual_seed(8)
    enc = bb.get_encoder("densenet121", weights="imagenet")
    assert enc.loaded_weights == str(f) and list(enc.state_dict()) == list(sd)
    assert all(torch.equal(v, sd[k]) for k, v in enc.state_dict().items())
    torch.save({**{k: v for k, v in sd.items()}, "classifier.bias": torch.zeros(1000)}, f)      # the current names load as they are
    assert all(torch.equal(v, sd[k]) for k, v in bb.get_encoder("densenet121", weights="imagenet").state_dict().items())
    with pytest.raises(RuntimeError):
        bb.get_encoder("densenet169", weights="imagenet")          # strict loading: another encoder's file is refused


def test_preprocessing_params_answer_the_names():
    from fastposecnn_amd.tools import dataset
    for name in NAMES:
        assert dataset.get_preprocessing_params(name) == dataset.get_preprocessing_params("resnet18")
    with pytest.raises(ValueError):
        dataset.get_preprocessing_params("densenet161")


@pytest.mark.parametrize("name", NAMES)
def test_engine_param_table_matches_state_dict(hiplib, name):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = name
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    h = ctypes.c_void_p()
    assert hiplib.fpc_net_create(name.encode(), 7, 2, 480, 640, ctypes.byref(h)) == 0
    try:
        n = hiplib.fpc_net_param_count(h)
        names = [hiplib.fpc_net_param_name(h, i).decode() for i in range(n)]
        assert len(set(names)) == n
        for i, nm in enumerate(names):
            assert nm in sd, nm
            assert sd[nm].numel() == hiplib.fpc_net_param_numel(h, i), nm
        assert [k for k in sd if k not in set(names) and not k.endswith("num_batches_tracked")] == []
        order = [k for k in m.state_dict() if k.startswith("encoder.") and not k.endswith("num_batches_tracked")]
        assert [nm for nm in names if nm.startswith("encoder.")] == order and len(order) == KEYS[name] - (2 * sum(BLOCKS[name]) + 5)
        assert sum(hiplib.fpc_net_param_numel(h, i) for i, nm in enumerate(names)
                   if nm.startswith("encoder.") and not nm.endswith(("running_mean", "running_var"))) == PARAMS[name]
        assert names.index("mask_decoder.p5.weight") == len(order)         # then the decoders and heads, as on every plan
        assert hiplib.fpc_net_workspace_bytes(h) > 0
        assert hiplib.fpc_net_forward(h, *([None] * 11), None) == -1          # before load_params: refused, not a crash
        assert hiplib.fpc_net_force_fold(h, 1) == -1 and hiplib.fpc_net_force_fold(h, 0) == 0
        assert hiplib.fpc_net_force_direct_h3(h, 1) == -1                     # (no three-product image is packed before a load)
        # the convolution sites are the stem and the decoders' 4 x (4 laterals + 7 segmentation convolutions); the laterals read c5 .. c2
        out = (ctypes.c_int * 5)()
        plans = []
        for i in range(hiplib.fpc_net_conv_count(h)):
            assert hiplib.fpc_net_conv_plan(h, i, out) == 0
            plans.append(tuple(out))
        assert len(plans) == 45 and plans[0][3:] == (64, 224)
        assert [p[4] for p in plans[1:5]] == list(OUT[name][:1:-1]) and all(p[3] == 256 for p in plans[1:5])
        # FLOP of a frame: the dense ops by arithmetic beside what the stem, the decoder sites and the heads count
        fl = (ctypes.c_double * 3)()
        assert hiplib.fpc_net_flops(h, fl) == 0
        hw, c, macs = 120 * 160, 64, 0
        for b, layers in enumerate(BLOCKS[name]):
            for _ in range(layers):
                macs += hw * (c * 128 + 1152 * 32)
                c += 32
            if b < 3:
                hw //= 4
                macs += hw * c * (c // 2)      # (the plan pools first: the conv runs on a quarter of the pixels)
                c //= 2
        stem = 240 * 320 * 64 * 147
        cs = OUT[name]
        dec = sum(2.0 * 2 * hwl * 256 * cin * 4 for hwl, cin in ((300, cs[5]), (1200, cs[4]), (4800, cs[3]), (19200, cs[2])))
        dec += sum(2.0 * 2 * hwl * 128 * cin * 9 * 4 for hwl, cin in ((300, 256), (1200, 128), (4800, 128), (1200, 256), (4800, 128),
                                                                     (4800, 256), (19200, 256)))
        heads = sum(2.0 * 2 * 19200 * 128 * ch for ch in (7, 24, 18, 18))
        assert fl[0] == 2.0 * 2 * (macs + stem) + dec + heads
        if name == "densenet121":              # the hot path: the 3x3 layers are 15 of the encoder's 30 GFLOP at 640 x 480
            conv2 = sum(2.0 * 1152 * 32 * layers * (19200 >> (2 * b)) for b, layers in enumerate(BLOCKS[name]))
            assert 14e9 < conv2 < 16e9 and 28e9 < 2.0 * (macs + stem) < 32e9
    finally:
        hiplib.fpc_net_destroy(h)


def test_engine_refusals(hiplib):
    h = ctypes.c_void_p()
    for name in NAMES:
        assert hiplib.fpc_net_create(name.encode(), 7, 2, 481, 640, ctypes.byref(h)) == -1
        assert hiplib.fpc_net_create(name.encode(), 1, 2, 480, 640, ctypes.byref(h)) == -1
        assert hiplib.fpc_net_create(name.encode(), 33, 2, 480, 640, ctypes.byref(h)) == -1
        assert hiplib.fpc_net_create(name.encode(), 7, 0, 480, 640, ctypes.byref(h)) == -1
    for name in (b"densenet161", b"densenet", b"densenet121 ", b"densenet-121"):
        assert hiplib.fpc_net_create(name, 7, 1, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(b"densenet201", 32, 1, 32, 32, ctypes.byref(h)) == 0
    hiplib.fpc_net_destroy(h)
    assert hiplib.fpc_abi_version() == 11


def test_standalone_entries_refuse_bad_arguments_on_the_host(hiplib):
    """Everything the entries check before they launch: no device memory is touched (the 'pointers' are aligned integers)."""
    L = hiplib
    p = [4096 * (i + 1) for i in range(7)]
    pick = lambda base, kw, keys: [{**base, **kw}[k] for k in keys]
    # in, s1, t1, w, s2, t2, out
    pw = lambda a=None, **kw: L.fpc_dense_pw(*(a or p), *pick(dict(M=300, K=96, Cout=128, ldi=256, ldo=128, act=1, form=-1), kw,
                                                              ("M", "K", "Cout", "ldi", "ldo", "act", "form")), None)
    for bad in (dict(K=48), dict(K=0), dict(K=2080), dict(Cout=48), dict(Cout=0), dict(Cout=1056), dict(ldi=64), dict(ldi=95), dict(ldi=98),
                dict(ldo=127), dict(ldo=96), dict(M=0), dict(M=2 ** 31 - 64), dict(act=2), dict(act=-1), dict(form=2), dict(form=-2)):
        assert pw(**bad) == -1, bad
    for i in (0, 3, 6):
        a = list(p); a[i] = None
        assert pw(a) == -1, ("null", i)
    for i in range(7):
        a = list(p); a[i] = p[i] + 4
        assert pw(a) == -1, ("misaligned", i)
    for i, j in ((1, 2), (4, 5)):                                    # an affine is a scale AND a shift
        a = list(p); a[i] = None
        assert pw(a) == -1, ("half an affine", i)
        a = list(p); a[j] = None
        assert pw(a) == -1, ("half an affine", j)
    assert [L.fpc_dense_pw_form(m, k, co) for m, k, co in ((300, 1024, 128), (1200, 512, 128), (4800, 256, 128), (19200, 64, 128),
                                                           (9600, 1024, 128), (300, 1024, 512), (4800, 256, 1024))] == [0, 0, 0, 1, 1, 0, 1]
    assert L.fpc_dense_pw_form(0, 64, 32) == -1 and L.fpc_dense_pw_form(300, 48, 32) == -1 and L.fpc_dense_pw_form(300, 64, 16) == -1
    assert L.fpc_dense_pw_form(300, 2048, 1024) == 0 and L.fpc_dense_pw_form(300, 2080, 1024) == -1
    # in, wt, out
    cv = lambda a=None, **kw: L.fpc_dense_conv3x3(*(a or p[:3]), *pick(dict(B=1, H=15, W=20, c0=224, ldo=256, form=-1), kw,
                                                                       ("B", "H", "W", "c0", "ldo", "form")), None)
    for bad in (dict(c0=225), dict(c0=16), dict(c0=-32), dict(c0=256), dict(ldo=255), dict(c0=0, ldo=31), dict(B=0), dict(H=0), dict(W=0),
                dict(form=2), dict(form=-2), dict(B=2 ** 15, H=2 ** 8, W=2 ** 8)):
        assert cv(**bad) == -1, bad
    for i in range(3):
        a = list(p[:3]); a[i] = None
        assert cv(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert cv(a) == -1, ("misaligned", i)
    assert L.fpc_dense_conv3x3_pack(None, p[1], None) == -1 and L.fpc_dense_conv3x3_pack(p[0], None, None) == -1
    assert L.fpc_dense_conv3x3_pack(p[0] + 4, p[1], None) == -1 and L.fpc_dense_conv3x3_pack(p[0], p[1] + 8, None) == -1
    assert L.fpc_dense_conv3x3_form(0, 4, 4) == -1 and L.fpc_dense_conv3x3_form(1, 0, 4) == -1 and L.fpc_dense_conv3x3_form(2 ** 15, 2 ** 8, 2 ** 8) == -1
    assert [L.fpc_dense_conv3x3_form(b, h, w) for b, h, w in ((1, 120, 160), (32, 120, 160), (32, 15, 20), (4, 120, 160))] == [0, 1, 0, 1]
    # x, s, t, skip, pooled
    npl = lambda a=None, **kw: L.fpc_dense_norm_pool(*(a or p[:5]), *pick(dict(B=1, H=6, W=10, C=256, act=1), kw, ("B", "H", "W", "C", "act")), None)
    for bad in (dict(H=5), dict(W=9), dict(C=6), dict(C=0), dict(C=2), dict(B=0), dict(H=0), dict(W=0), dict(act=2), dict(act=-1),
                dict(B=2 ** 10, H=2 ** 10, W=2 ** 10, C=64)):
        assert npl(**bad) == -1, bad
    for i in range(4):
        a = list(p[:5]); a[i] = None
        assert npl(a) == -1, ("null", i)
    for i in range(5):
        a = list(p[:5]); a[i] = p[i] + 4
        assert npl(a) == -1, ("misaligned", i)
    pl = lambda a=None, **kw: L.fpc_dense_place(*(a or p[:2]), *pick(dict(M=4800, C=64, ld=256), kw, ("M", "C", "ld")), None)
    for bad in (dict(M=0), dict(C=0), dict(C=6), dict(ld=60), dict(ld=66), dict(M=2 ** 40)):
        assert pl(**bad) == -1, bad
    for i in range(2):
        a = list(p[:2]); a[i] = None
        assert pl(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert pl(a) == -1, ("misaligned", i)


@pytest.mark.parametrize("B,H,W", D.SMALL_SHAPES)
def test_the_engine_tests_draw_is_well_conditioned(B, H, W):
    """What tests/test_gpu_densenet.py::test_engine_vs_float64_cpu asks of its own inputs: with its parameter draw, torch's f32 CPU
    forward of the module stays within a quarter of the network bar 1e-4 max(1, |ref|max) of float64 on c2 .. c5 and every logit, so
    the bar measures the engine and not the conditioning of the draw."""
    import fastposecnn_amd.lib as L
    for err, scale in BF.f32_errors(L, "densenet121", D.images(B, H, W)):
        assert err <= 0.25 * 1e-4 * max(1.0, scale), err


def test_the_batch_tests_frames_are_well_conditioned():
    """The same condition on what tests/test_gpu_batch_forms.py compares: frames 0, 17 and 31 of its batch at 352 x 416."""
    import fastposecnn_amd.lib as L
    x = BF.frames("densenet121")
    assert tuple(x.shape) == (3, 3, 352, 416)
    for err, scale in BF.f32_errors(L, "densenet121", x):
        assert err <= 0.25 * 1e-4 * max(1.0, scale), err
