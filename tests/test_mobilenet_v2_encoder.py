"""CPU checks of the MobileNetV2 encoder (mobilenet_v2): the module restatement against the published definition of torchvision's
MobileNetV2 as smp's MobileNetV2Encoder wraps it (parameter count by plain arithmetic, state-dict names against a committed manifest,
where the strides and the residuals sit, the block formula), checkpoint and encoder-weights loading, the preprocessing parameters,
the engine's host-side plan (fpc_net_create("mobilenet_v2"): parameter table, refusals) and the host-side refusals of the three
stand-alone kernel entries.  No compute calls into the HIP library."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
PARAMS = 2_223_872          # the published 3 504 872 minus the classifier's 1280 x 1000 + 1000


def encoder_params():
    """Parameters of the features by plain arithmetic: a convolution's weights and the BatchNorm's weight + bias behind each."""
    total = 32 * 3 * 9 + 2 * 32
    inp = 32
    for t, c, n, _ in SETTING:
        for _ in range(n):
            hid = inp * t
            if t != 1:
                total += hid * inp + 2 * hid
            total += hid * 9 + 2 * hid + c * hid + 2 * c
            inp = c
    return total + 1280 * inp + 2 * 1280


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


@pytest.fixture(scope="module")
def enc():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(0)
    return bb.get_encoder("mobilenet_v2")


def test_parameter_count(enc):
    assert PARAMS == 3_504_872 - 1_281_000
    assert encoder_params() == PARAMS
    assert sum(p.numel() for p in enc.parameters()) == PARAMS


def test_state_dict_key_order_equals_the_manifest(enc):
    """The manifest is written by tests/golden/make_state_dict_keys_mobilenet_v2.py from the published definition, not dumped from
    this module."""
    want = open(os.path.join(HERE, "golden", "state_dict_keys_mobilenet_v2.txt")).read().split()
    assert len(want) == 312
    assert list(enc.state_dict()) == want
    assert not any(k.startswith("classifier") for k in want)


def test_module_properties(enc):
    from fastposecnn_amd.lib import backbone as bb
    assert isinstance(enc, bb.MobileNetV2Encoder) and enc.name == "mobilenet_v2"
    assert enc.out_channels == (3, 16, 24, 32, 96, 1280)
    assert bb.encoder_family("mobilenet_v2") == "mobilenet_v2" and bb.encoder_family("resnet18") == "resnet"
    assert bb.encoder_layout("resnet18") == (1, [2, 2, 2, 2]) and bb.encoder_groups("resnext50_32x4d") == (32, 4)
    assert bb.encoder_reduction("se_resnet50") == 16
    with pytest.raises(KeyError):
        bb.encoder_family("mobilenet_v3")
    assert not hasattr(enc, "classifier") and len(enc.features) == 19
    with torch.no_grad():
        feats = enc.eval()(torch.randn(1, 3, 64, 96))
    assert [tuple(f.shape[1:]) for f in feats] == [(3, 64, 96), (16, 32, 48), (24, 16, 24), (32, 8, 12), (96, 4, 6), (1280, 2, 3)]
    assert all(torch.isfinite(f).all() for f in feats)
    # the stem and the last 1x1
    stem, last = enc.features[0], enc.features[18]
    assert stem[0].kernel_size == (3, 3) and stem[0].stride == (2, 2) and stem[0].padding == (1, 1) and stem[0].out_channels == 32
    assert last[0].kernel_size == (1, 1) and (last[0].in_channels, last[0].out_channels) == (320, 1280)
    assert isinstance(stem[2], torch.nn.ReLU6) and isinstance(last[2], torch.nn.ReLU6)
    # the blocks: strides, residuals, depthwise groups
    want = [(t, c, s if i == 0 else 1) for t, c, n, s in SETTING for i in range(n)]
    blocks = list(enc.features[1:18])
    assert len(blocks) == len(want) == 17
    inp, strided, residual = 32, [], []
    for idx, (blk, (t, c, s)) in enumerate(zip(blocks, want), start=1):
        hid = inp * t
        dw = blk.conv[0 if t == 1 else 1]
        assert len(blk.conv) == (3 if t == 1 else 4)
        assert dw[0].groups == hid == dw[0].in_channels == dw[0].out_channels and dw[0].stride == (s, s) and dw[0].kernel_size == (3, 3)
        assert isinstance(dw[2], torch.nn.ReLU6)
        if t != 1:
            assert blk.conv[0][0].kernel_size == (1, 1) and (blk.conv[0][0].in_channels, blk.conv[0][0].out_channels) == (inp, hid)
        proj = blk.conv[-2]
        assert proj.kernel_size == (1, 1) and (proj.in_channels, proj.out_channels) == (hid, c) and proj.stride == (1, 1)
        assert isinstance(blk.conv[-1], bb.BatchNorm2d)
        assert blk.use_res_connect == (s == 1 and inp == c)
        if s == 2:
            strided.append(idx)
        if blk.use_res_connect:
            residual.append(idx)
        inp = c
    assert strided == [2, 4, 7, 14]
    assert residual == [3, 5, 6, 8, 9, 10, 12, 13, 15, 16] and len(residual) == 10
    convs = [m for m in enc.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 52 and all(isinstance(m, bb.Conv2d) and m.bias is None for m in convs)
    assert all(isinstance(m, bb.BatchNorm2d) for m in enc.modules() if isinstance(m, torch.nn.BatchNorm2d))


def _relu6(v):
    return v.clamp(0.0, 6.0)


def _bn(v, bn):
    sh = (1, -1, 1, 1)
    return (v - bn.running_mean.view(sh)) / torch.sqrt(bn.running_var.view(sh) + bn.eps) * bn.weight.view(sh) + bn.bias.view(sh)


@pytest.mark.parametrize("idx", [3, 1], ids=["t6-residual", "t1"])
def test_block_forward_is_the_published_formula(idx):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(3)
    e = bb.get_encoder("mobilenet_v2")
    g = torch.Generator().manual_seed(idx)
    for m in e.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    blk = e.features[idx].eval().double()
    c = blk.conv
    inp = c[0][0].in_channels
    x = torch.randn(2, inp, 6, 10, dtype=torch.float64) * 3.0
    with torch.no_grad():
        v = x
        k = 0
        if idx != 1:
            v = _relu6(_bn(F.conv2d(v, c[0][0].weight), c[0][1]))
            k = 1
        hid = v.shape[1]
        v = _relu6(_bn(F.conv2d(v, c[k][0].weight, None, 1, 1, 1, hid), c[k][1]))
        v = _bn(F.conv2d(v, c[k + 1].weight), c[k + 2])
        want = x + v if idx != 1 else v
        got = blk(x)
    assert blk.use_res_connect == (idx != 1)
    assert (got < 0).any()                                         # no activation behind the add / the projection
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_load_from_ckpt_mobilenet_v2_round_trip(tmp_path):
    """A Lightning-style checkpoint whose hyper-parameters name mobilenet_v2 loads (KeyError before) and reproduces the donor's
    logits bit for bit."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config, synth
    hp_src = config.HEAD_TRAINING()
    hp_src.ENCODER = 'mobilenet_v2'
    torch.manual_seed(5)
    src = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp_src).eval()
    ckpt = {'state_dict': {'model.' + k: v.clone() for k, v in src.state_dict().items()},
            'hyper_parameters': {'MODEL': 'PoseRegressor', 'BACKBONE_ARCH': 'FPN', 'ENCODER': 'mobilenet_v2',
                                 'ENCODER_WEIGHTS': None, 'SELECTED_CLASSES': hp_src.SELECTED_CLASSES}}
    path = tmp_path / "last.ckpt"
    torch.save(ckpt, path)
    hp = config.INFERENCE()
    torch.manual_seed(77)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(str(path), hp).eval()
    assert hp.ENCODER == 'mobilenet_v2' and m.encoder.name == 'mobilenet_v2'
    sd, want = m.state_dict(), src.state_dict()
    assert list(sd) == list(want)
    assert "encoder.features.0.0.weight" in sd and "encoder.features.2.conv.1.1.running_var" in sd and "encoder.features.18.1.bias" in sd
    assert tuple(sd["mask_decoder.p2.skip_conv.weight"].shape) == (256, 24, 1, 1)
    assert tuple(sd["mask_decoder.p5.weight"].shape) == (256, 1280, 1, 1)
    for k in want:
        assert torch.equal(sd[k], want[k]), k
    x = synth.make_image(0, 64, 64)[None]
    hp.PERFORM_AGGREGATION = False
    hp_src.PERFORM_AGGREGATION = False
    with torch.no_grad():
        a, b = m(x), src(x)
    for k in a["logits"]:
        assert torch.equal(a["logits"][k], b["logits"][k]), k


def test_encoder_weights_file_with_classifier(tmp_path, monkeypatch):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(4)
    donor = bb.MobileNetV2Encoder()
    tv = {k: v.clone() for k, v in donor.state_dict().items()}
    tv['classifier.1.weight'] = torch.zeros(1000, 1280); tv['classifier.1.bias'] = torch.zeros(1000)
    f = tmp_path / "mobilenet_v2.pth"
    torch.save(tv, f)
    monkeypatch.setenv("FPC_ENCODER_WEIGHTS", str(f))
    torch.manual_seed(8)
    enc = bb.get_encoder('mobilenet_v2', weights='imagenet')
    assert enc.loaded_weights == str(f)
    assert all(torch.equal(v, donor.state_dict()[k]) for k, v in enc.state_dict().items())
    with pytest.raises(RuntimeError):
        bb.get_encoder('resnet18', weights='imagenet')          # a MobileNetV2 file is not a ResNet file ...
    r = tmp_path / "resnet18.pth"
    torch.save(bb.ResNetEncoder('resnet18').state_dict(), r)
    monkeypatch.setenv("FPC_ENCODER_WEIGHTS", str(r))
    with pytest.raises(RuntimeError):
        bb.get_encoder('mobilenet_v2', weights='imagenet')      # ... and a ResNet file is refused: strict loading


def test_preprocessing_params_answer_the_name():
    from fastposecnn_amd.tools import dataset
    assert dataset.get_preprocessing_params("mobilenet_v2") == dataset.get_preprocessing_params("resnet18")
    with pytest.raises(ValueError):
        dataset.get_preprocessing_params("mobilenet_v3_large")


def test_engine_param_table_matches_state_dict(hiplib):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = "mobilenet_v2"
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    h = ctypes.c_void_p()
    assert hiplib.fpc_net_create(b"mobilenet_v2", 7, 2, 480, 640, ctypes.byref(h)) == 0
    try:
        n = hiplib.fpc_net_param_count(h)
        names = [hiplib.fpc_net_param_name(h, i).decode() for i in range(n)]
        assert len(set(names)) == n
        for i, nm in enumerate(names):
            assert nm in sd, nm
            assert sd[nm].numel() == hiplib.fpc_net_param_numel(h, i), nm
        unused = [k for k in sd if k not in set(names) and not k.endswith("num_batches_tracked")]
        assert unused == []
        order = [k for k in m.state_dict() if k.startswith("encoder.") and not k.endswith("num_batches_tracked")]
        assert [nm for nm in names if nm.startswith("encoder.")] == order and len(order) == 260
        assert names.index("mask_decoder.p5.weight") == 260                   # then the decoders and heads, as on every plan
        assert hiplib.fpc_net_workspace_bytes(h) > 0
        assert hiplib.fpc_net_forward(h, *([None] * 11), None) == -1          # before load_params: refused, not a crash
        assert hiplib.fpc_net_force_stem_pool(h, 1) == -1 and hiplib.fpc_net_force_stem_pool(h, 0) == -1
        assert hiplib.fpc_net_force_fold(h, 1) == -1 and hiplib.fpc_net_force_fold(h, 0) == 0
        # the convolution sites are the decoders' alone: 4 x (4 laterals + 7 segmentation convolutions); the laterals read 1280 / 96 /
        # 32 / 24 channels
        out = (ctypes.c_int * 5)()
        plans = []
        for i in range(hiplib.fpc_net_conv_count(h)):
            assert hiplib.fpc_net_conv_plan(h, i, out) == 0
            plans.append(tuple(out))
        assert len(plans) == 44
        assert [p[4] for p in plans[:4]] == [1280, 96, 32, 24] and all(p[3] == 256 for p in plans[:4])
        # FLOP of a frame: the encoder's 52 ops by arithmetic + what the decoder sites and heads count
        fl = (ctypes.c_double * 3)()
        assert hiplib.fpc_net_flops(h, fl) == 0
        enc_macs = 240 * 320 * 32 * 27
        inp, hw = 32, 240 * 320
        for t, c, nb, s in SETTING:
            for i in range(nb):
                hid = inp * t
                if t != 1:
                    enc_macs += hw * inp * hid
                if i == 0 and s == 2:
                    hw //= 4
                enc_macs += hw * hid * 9 + hw * hid * c
                inp = c
        enc_macs += hw * 320 * 1280
        assert hw == 15 * 20 and 1.8e9 < enc_macs < 1.9e9
        dec = sum(2.0 * 2 * hwl * 256 * cin * 4 for hwl, cin in ((300, 1280), (1200, 96), (4800, 32), (19200, 24)))
        dec += sum(2.0 * 2 * hwl * 128 * cin * 9 * 4 for hwl, cin in ((300, 256), (1200, 128), (4800, 128), (1200, 256), (4800, 128),
                                                                     (4800, 256), (19200, 256)))
        heads = sum(2.0 * 2 * 19200 * 128 * ch for ch in (7, 24, 18, 18))
        assert fl[0] == fl[1] == 2.0 * 2 * enc_macs + dec + heads and fl[2] == 0.0
    finally:
        hiplib.fpc_net_destroy(h)


def test_engine_refusals(hiplib):
    h = ctypes.c_void_p()
    assert hiplib.fpc_net_create(b"mobilenet_v2", 7, 2, 481, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(b"mobilenet_v2", 7, 2, 480, 650, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(b"mobilenet_v2", 1, 2, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(b"mobilenet_v2", 33, 2, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(b"mobilenet_v2", 7, 0, 480, 640, ctypes.byref(h)) == -1
    for name in (b"mobilenet_v3", b"mobilenet_v2_", b"mobilenet"):
        assert hiplib.fpc_net_create(name, 7, 1, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(b"mobilenet_v2", 32, 1, 32, 32, ctypes.byref(h)) == 0
    hiplib.fpc_net_destroy(h)
    assert hiplib.fpc_abi_version() == 11


def test_standalone_entries_refuse_bad_arguments_on_the_host(hiplib):
    """Everything the entries check before they launch: no device memory is touched (the 'pointers' are aligned integers)."""
    L = hiplib
    p = [4096 * (i + 1) for i in range(6)]
    dw = lambda a=None, **kw: L.fpc_dwconv3x3(*(a or p[:5]), *[{**dict(B=1, Hi=4, Wi=4, C=32, stride=1, act=1), **kw}[k] for k in ("B", "Hi", "Wi", "C", "stride", "act")], None)
    for bad in (dict(C=6), dict(C=0), dict(C=2), dict(stride=3), dict(stride=0), dict(B=0), dict(act=2), dict(act=-1), dict(Hi=0), dict(Wi=0)):
        assert dw(**bad) == -1, bad
    for i in range(5):
        a = list(p[:5]); a[i] = None
        assert dw(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert dw(a) == -1, ("misaligned", i)
    pw = lambda a=None, **kw: L.fpc_conv1x1_f32(*(a or p[:4] + [None, p[5]]), *[{**dict(M=6, Cin=16, Cout=96, act=0), **kw}[k] for k in ("M", "Cin", "Cout", "act")], None)
    for bad in (dict(Cin=12), dict(Cin=0), dict(Cin=1032), dict(Cout=12), dict(Cout=4), dict(Cout=2056), dict(M=0), dict(act=2), dict(act=6)):
        assert pw(**bad) == -1, bad
    assert pw(p[:6], act=1) == -1                                  # a residual together with an activation
    for i in (0, 1, 2, 3, 5):
        a = p[:4] + [None, p[5]]; a[i] = None
        assert pw(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert pw(a) == -1, ("misaligned", i)
    assert pw(p[:4] + [p[4] + 4, p[5]]) == -1                      # a misaligned residual
    # the form of a 1x1 site, a function of the shape alone: 16 x 16 tiles below 1024 tiles of 32 x 32, else 5 / 3 / 2 channel tiles per
    # wave where they divide the site's and leave 2048 waves, else 1
    assert [L.fpc_conv1x1_f32_form(m, 32, co) for m, co in ((300, 160), (32 * 1023, 8), (32 * 1023 + 1, 8), (9600, 160), (76800, 96),
                                                            (32 * 2048, 96), (32 * 2048, 64), (32 * 2048, 160), (32 * 2048, 128),
                                                            (2457600, 16), (19200, 144))] == [0, 0, 1, 1, 3, 3, 2, 5, 2, 1, 1]
    assert L.fpc_conv1x1_f32_form(0, 32, 16) == -1 and L.fpc_conv1x1_f32_form(300, 12, 16) == -1 and L.fpc_conv1x1_f32_form(300, 32, 4) == -1
    st = lambda a=None, **kw: L.fpc_stem3x3s2(*(a or p[:5]), *[{**dict(B=1, Hi=4, Wi=4, Cout=32), **kw}[k] for k in ("B", "Hi", "Wi", "Cout")], None)
    for bad in (dict(Cout=64), dict(Cout=16), dict(B=0), dict(Hi=0), dict(Wi=0)):
        assert st(**bad) == -1, bad
    for i in range(5):
        a = list(p[:5]); a[i] = None
        assert st(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert st(a) == -1, ("misaligned", i)
