"""CPU checks of the SE-ResNet encoders (se_resnet50 / 101 / 152): the module restatement against the published definition of
smp's SENetEncoder over pretrainedmodels.senet (parameter counts by plain arithmetic, state-dict names against a committed manifest,
where the stride sits, the ceil-mode stem pool), checkpoint and encoder-weights loading, and the engine's host-side plan
(fpc_net_create_encoder_se: parameter table, refusals).  No compute calls into the HIP library."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
LAYERS = {"se_resnet50": [3, 4, 6, 3], "se_resnet101": [3, 4, 23, 3], "se_resnet152": [3, 8, 36, 3]}
# the published totals (28 088 024 / 49 326 872 / 66 821 848) minus the 2 049 000 parameters of `last_linear`
PARAMS = {"se_resnet50": 26_039_024, "se_resnet101": 47_277_872, "se_resnet152": 64_772_848}
RESNET = {"se_resnet50": 23_508_032, "se_resnet101": 42_500_160, "se_resnet152": 58_143_808}      # ResNet-50 / 101 / 152 without `fc`


def resnet_encoder_params(layers):
    """Parameters of a Bottleneck ResNet without `fc`: the stem (7x7 conv + BN) and per block 1x1 -> 3x3 -> 1x1 x 4, a BatchNorm
    (weight + bias) behind each, and on block 0 of a stage the 1x1 downsample + BN.  (Where the stride sits changes no count.)"""
    total = 64 * 3 * 49 + 2 * 64
    inpl = 64
    for planes, n in zip((64, 128, 256, 512), layers):
        for b in range(n):
            total += inpl * planes + 2 * planes + planes * planes * 9 + 2 * planes + planes * 4 * planes + 2 * 4 * planes
            if b == 0:
                total += inpl * 4 * planes + 2 * 4 * planes
            inpl = 4 * planes
    return total


def se_params(layers):
    """... plus, per block of C = 4 planes channels, fc1 (C x C / 16 + C / 16) and fc2 (C / 16 x C + C): 2 C^2 / 16 + C / 16 + C."""
    return resnet_encoder_params(layers) + sum(n * (2 * C * C // 16 + C // 16 + C) for C, n in zip((256, 512, 1024, 2048), layers))


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def test_arithmetic_gives_the_published_totals():
    for name in PARAMS:
        assert resnet_encoder_params(LAYERS[name]) == RESNET[name], name
        assert se_params(LAYERS[name]) == PARAMS[name], name


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_encoder_parameter_count_channels_and_lookups(name):
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder(name)
    assert isinstance(enc, bb.SENetEncoder) and enc.name == name
    assert sum(p.numel() for p in enc.parameters()) == PARAMS[name]
    assert enc.out_channels == (3, 64, 256, 512, 1024, 2048)
    assert bb.encoder_layout(name) == (4, LAYERS[name])
    assert bb.encoder_groups(name) == (1, 64)
    assert bb.encoder_reduction(name) == 16
    for other in ("resnet18", "resnet34", "resnet50", "resnext50_32x4d", "resnext101_32x8d"):
        assert bb.encoder_reduction(other) == 0
    with pytest.raises(KeyError):
        bb.encoder_reduction("se_resnext50_32x4d")
    for L, n in enumerate(LAYERS[name]):
        assert len(getattr(enc, f"layer{L + 1}")) == n


def test_state_dict_key_order_equals_the_manifest():
    """The manifest was written from pretrainedmodels' published SENet / SEResNetBottleneck / SEModule definitions (attribute order:
    conv1, bn1, conv2, bn2, conv3, bn3, relu, se_module, downsample), not dumped from this module."""
    from fastposecnn_amd.lib import backbone as bb
    want = open(os.path.join(HERE, "golden", "state_dict_keys_se_resnet50.txt")).read().split()
    assert len(want) == 382
    assert list(bb.get_encoder("se_resnet50").state_dict()) == want


def test_stride_on_conv1_and_downsample_only_and_biased_gate():
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder("se_resnet50")
    for L in range(1, 5):
        layer = getattr(enc, f"layer{L}")
        s = 1 if L == 1 else 2
        C = 64 * 2 ** (L - 1) * 4
        assert layer[0].conv1.stride == (s, s) and layer[0].conv1.kernel_size == (1, 1)
        assert layer[0].downsample is not None and layer[0].downsample[0].stride == (s, s)
        assert layer[0].downsample[0].kernel_size == (1, 1) and layer[0].downsample[0].bias is None
        assert all(blk.downsample is None and blk.conv1.stride == (1, 1) for blk in layer[1:])
        for blk in layer:
            assert blk.conv2.stride == (1, 1) and blk.conv2.kernel_size == (3, 3) and blk.conv2.padding == (1, 1)
            assert blk.conv2.groups == 1 and blk.conv3.out_channels == C and blk.conv3.kernel_size == (1, 1)
            assert all(isinstance(c, bb.Conv2d) and c.bias is None for c in (blk.conv1, blk.conv2, blk.conv3))
            assert all(isinstance(b, bb.BatchNorm2d) for b in (blk.bn1, blk.bn2, blk.bn3))
            se = blk.se_module
            assert type(se.fc1) is torch.nn.Conv2d and type(se.fc2) is torch.nn.Conv2d          # plain modules in every mode
            assert tuple(se.fc1.weight.shape) == (C // 16, C, 1, 1) and tuple(se.fc2.weight.shape) == (C, C // 16, 1, 1)
            assert tuple(se.fc1.bias.shape) == (C // 16,) and tuple(se.fc2.bias.shape) == (C,)


def test_block_forward_is_the_published_formula():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(3)
    blk = bb.get_encoder("se_resnet50").layer2[0].eval().double()
    x = torch.randn(2, 256, 6, 10, dtype=torch.float64)
    with torch.no_grad():
        out = blk.bn3(blk.conv3(blk.bn2(blk.conv2(blk.bn1(blk.conv1(x)).relu())).relu()))
        m = out.mean(dim=(2, 3), keepdim=True)
        se = blk.se_module
        g = torch.sigmoid(F.conv2d(F.conv2d(m, se.fc1.weight, se.fc1.bias).relu(), se.fc2.weight, se.fc2.bias))
        want = (out * g + blk.downsample(x)).relu()
        assert torch.allclose(blk(x), want, rtol=0, atol=1e-12)


def test_stem_pool_is_ceil_mode_without_padding():
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder("se_resnet50")
    assert list(dict(enc.layer0.named_children())) == ["conv1", "bn1", "relu1", "pool"]
    pool = enc.layer0.pool
    assert type(pool) is torch.nn.MaxPool2d          # never the pad-1 native training kernels
    assert pool.ceil_mode and pool.padding in (0, (0, 0)) and pool.kernel_size in (3, (3, 3)) and pool.stride in (2, (2, 2))
    assert enc.layer0.conv1.kernel_size == (7, 7) and enc.layer0.conv1.stride == (2, 2) and enc.layer0.conv1.padding == (3, 3)
    assert enc.layer0.conv1.bias is None
    torch.manual_seed(0)
    x = torch.randn(1, 4, 8, 12)
    a, b = pool(x), F.max_pool2d(x, 3, 2, 1)
    assert a.shape == b.shape == (1, 4, 4, 6) and not torch.equal(a, b)
    assert torch.equal(a[0, :, 0, 0], x[0, :, 0:3, 0:3].amax(dim=(1, 2)))           # windows start at 0
    assert torch.equal(a[0, :, 3, 5], x[0, :, 6:8, 10:12].amax(dim=(1, 2)))         # the last one is clipped
    for h, w in ((2, 2), (16, 24), (32, 48), (240, 320)):
        assert pool(torch.zeros(1, 1, h, w)).shape == (1, 1, h // 2, w // 2)


def test_feature_shapes():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(0)
    enc = bb.get_encoder("se_resnet50").eval()
    with torch.no_grad():
        feats = enc(torch.randn(1, 3, 64, 96))
    assert [tuple(f.shape) for f in feats] == [(1, 3, 64, 96), (1, 64, 32, 48), (1, 256, 16, 24), (1, 512, 8, 12),
                                                (1, 1024, 4, 6), (1, 2048, 2, 3)]
    assert all(torch.isfinite(f).all() for f in feats)


def test_se_resnext_is_still_refused():
    from fastposecnn_amd.lib import backbone as bb
    with pytest.raises(KeyError) as e:
        bb.get_encoder("se_resnext50_32x4d")
    assert "resnext50_32x4d" in str(e.value) and "se_resnet50" in str(e.value)
    with pytest.raises(KeyError):
        bb.encoder_layout("se_resnext50_32x4d")


def test_load_from_ckpt_se_resnet50_round_trip(tmp_path):
    """A Lightning-style checkpoint whose hyper-parameters name the SE-ResNet-50 encoder loads (KeyError before)."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config, synth
    hp_src = config.HEAD_TRAINING()
    hp_src.ENCODER = 'se_resnet50'
    torch.manual_seed(5)
    src = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp_src).eval()
    ckpt = {'state_dict': {'model.' + k: v.clone() for k, v in src.state_dict().items()},
            'hyper_parameters': {'MODEL': 'PoseRegressor', 'BACKBONE_ARCH': 'FPN', 'ENCODER': 'se_resnet50',
                                 'ENCODER_WEIGHTS': None, 'SELECTED_CLASSES': hp_src.SELECTED_CLASSES}}
    path = tmp_path / "last.ckpt"
    torch.save(ckpt, path)
    hp = config.INFERENCE()
    torch.manual_seed(77)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(str(path), hp).eval()
    assert hp.ENCODER == 'se_resnet50' and m.encoder.name == 'se_resnet50'
    sd, want = m.state_dict(), src.state_dict()
    assert list(sd) == list(want)
    assert any(k.endswith("se_module.fc2.bias") for k in sd)
    for k in want:
        assert torch.equal(sd[k], want[k]), k
    x = synth.make_image(0, 64, 64)[None]
    hp.PERFORM_AGGREGATION = False
    hp_src.PERFORM_AGGREGATION = False
    with torch.no_grad():
        a, b = m(x), src(x)
    for k in a["logits"]:
        assert torch.equal(a["logits"][k], b["logits"][k]), k


def test_encoder_weights_file_with_last_linear(tmp_path, monkeypatch):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(4)
    donor = bb.SENetEncoder('se_resnet50')
    pm = {k: v.clone() for k, v in donor.state_dict().items()}
    pm['last_linear.weight'] = torch.zeros(1000, 2048); pm['last_linear.bias'] = torch.zeros(1000)
    f = tmp_path / "se50.pth"
    torch.save(pm, f)
    monkeypatch.setenv("FPC_ENCODER_WEIGHTS", str(f))
    torch.manual_seed(8)
    enc = bb.get_encoder('se_resnet50', weights='imagenet')
    assert enc.loaded_weights == str(f)
    assert all(torch.equal(v, donor.state_dict()[k]) for k, v in enc.state_dict().items())
    with pytest.raises(RuntimeError):
        bb.get_encoder('resnet50', weights='imagenet')          # an SE-ResNet file is not a ResNet-50 file: strict loading


def test_preprocessing_params_answer_the_se_names():
    from fastposecnn_amd.tools import dataset
    assert dataset.get_preprocessing_params("se_resnet50") == dataset.get_preprocessing_params("resnet50")


def _create_se(hiplib, layers, reduction, classes=7, B=2, H=480, W=640):
    h = ctypes.c_void_p()
    rc = hiplib.fpc_net_create_encoder_se((ctypes.c_int * 4)(*layers), reduction, classes, B, H, W, ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_engine_param_table_matches_state_dict(hiplib, name):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = name
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    rc, h = _create_se(hiplib, LAYERS[name], 16)
    assert rc == 0
    g = ctypes.c_void_p()
    assert hiplib.fpc_net_create(name.encode(), 7, 2, 480, 640, ctypes.byref(g)) == 0       # the named entry answers it too
    try:
        n = hiplib.fpc_net_param_count(h)
        names = [hiplib.fpc_net_param_name(h, i).decode() for i in range(n)]
        assert len(set(names)) == n
        for i, nm in enumerate(names):
            assert nm in sd, nm
            assert sd[nm].numel() == hiplib.fpc_net_param_numel(h, i), nm
        unused = [k for k in sd if k not in set(names) and not k.endswith("num_batches_tracked")]
        assert unused == []
        # the encoder's part in state-dict order
        order = [k for k in m.state_dict() if k.startswith("encoder.") and not k.endswith("num_batches_tracked")]
        assert [nm for nm in names if nm.startswith("encoder.")] == order
        assert hiplib.fpc_net_param_count(g) == n and hiplib.fpc_net_workspace_bytes(g) == hiplib.fpc_net_workspace_bytes(h) > 0
        assert hiplib.fpc_net_forward(h, *([None] * 11), None) == -1       # before load_params: refused, not a crash
        # every conv2 is a 3x3 / stride-1 site: K = 9 planes, as many of them as blocks
        out = (ctypes.c_int * 5)()
        plans = []
        for i in range(hiplib.fpc_net_conv_count(h)):
            assert hiplib.fpc_net_conv_plan(h, i, out) == 0
            plans.append(tuple(out))
        enc_sites = 1 + 3 * sum(LAYERS[name]) + 4
        k3 = [p[4] for p in plans[1:enc_sites] if p[4] == 9 * p[3]]
        assert k3 == [9 * 64 * 2 ** L for L, cnt in enumerate(LAYERS[name]) for _ in range(cnt)]
        assert hiplib.fpc_net_force_stem_pool(h, 1) == -1                  # a pad-1 launch: refused on an SE plan
    finally:
        hiplib.fpc_net_destroy(h)
        hiplib.fpc_net_destroy(g)


def test_refusals_and_host_arithmetic(hiplib):
    R50 = [3, 4, 6, 3]
    for red in (0, -16, 3, 24, 48, 512):                                    # does not divide 256
        rc, _ = _create_se(hiplib, R50, red)
        assert rc == -1, red
    for red in (1, 4, 16, 32, 256):
        rc, h = _create_se(hiplib, R50, red, B=1, H=64, W=96)
        assert rc == 0, red
        hiplib.fpc_net_destroy(h)
    h = ctypes.c_void_p()
    assert hiplib.fpc_net_create_encoder_se(None, 16, 7, 1, 480, 640, ctypes.byref(h)) == -1
    assert _create_se(hiplib, R50, 16, H=481)[0] == -1
    assert _create_se(hiplib, [3, 4, 0, 3], 16)[0] == -1
    for name in (b"se_resnext50_32x4d", b"se_resnet18", b"senet154"):
        assert hiplib.fpc_net_create(name, 7, 1, 480, 640, ctypes.byref(h)) == -1
    # the slab count: a function of the shape, 0 for a refused one; scratch = B x slabs x C
    assert hiplib.fpc_se_pool_slabs(1, 1, 64) == 1 and hiplib.fpc_se_pool_slabs(37, 41, 128) > 1
    assert hiplib.fpc_se_pool_slabs(5, 7, 96) == 0 and hiplib.fpc_se_pool_slabs(0, 7, 64) == 0
    assert hiplib.fpc_se_scratch_floats(3, 37, 41, 128) == 3 * hiplib.fpc_se_pool_slabs(37, 41, 128) * 128
    assert hiplib.fpc_se_scratch_floats(0, 37, 41, 128) == 0


def test_abi_version_is_unchanged(hiplib):
    assert hiplib.fpc_abi_version() == 11
