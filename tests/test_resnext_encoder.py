"""CPU checks of the ResNeXt encoders (resnext50_32x4d, resnext101_32x4d, resnext101_32x8d): the module restatement against
torchvision's definition (parameter counts by plain arithmetic, shapes, names), checkpoint and encoder-weights loading, and the
engine's host-side plan (fpc_net_create_encoder_ex: parameter table, refusals, the grouped plan code at the conv2 sites).  No
compute calls into the HIP library."""
import ctypes

import pytest
import torch

LAYERS = {"resnext50_32x4d": [3, 4, 6, 3], "resnext101_32x4d": [3, 4, 23, 3], "resnext101_32x8d": [3, 4, 23, 3]}
WIDTHS = {"resnext50_32x4d": (32, 4), "resnext101_32x4d": (32, 4), "resnext101_32x8d": (32, 8)}
# torchvision's totals minus the 2 049 000 parameters of `fc`
PARAMS = {"resnext50_32x4d": 22_979_904, "resnext101_32x4d": 42_128_704, "resnext101_32x8d": 86_742_336}
FPC_PLAN_GROUPED = 8000


def tv_encoder_params(layers, groups, width_per_group):
    """Parameters of torchvision's ResNet(Bottleneck, layers, groups, width_per_group) without `fc`: the stem (7x7 conv + BN), and
    per block conv1 1x1 -> width, conv2 3x3 grouped, conv3 1x1 -> 4 planes, a BatchNorm (weight + bias) behind each, and on block 0
    of a stage the 1x1 downsample + BN."""
    total = 64 * 3 * 49 + 2 * 64
    inpl = 64
    for planes, n in zip((64, 128, 256, 512), layers):
        width = int(planes * width_per_group / 64) * groups
        for b in range(n):
            total += inpl * width + 2 * width
            total += width * (width // groups) * 9 + 2 * width
            total += width * 4 * planes + 2 * 4 * planes
            if b == 0:
                total += inpl * 4 * planes + 2 * 4 * planes
            inpl = 4 * planes
    return total


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def test_arithmetic_gives_torchvisions_totals():
    for name in PARAMS:
        assert tv_encoder_params(LAYERS[name], *WIDTHS[name]) == PARAMS[name], name
    assert tv_encoder_params([3, 4, 6, 3], 1, 64) == 23_508_032       # ResNet-50


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_encoder_parameter_count_and_channels(name):
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder(name)
    assert sum(p.numel() for p in enc.parameters()) == PARAMS[name]
    assert enc.out_channels == bb.get_encoder("resnet50").out_channels == (3, 64, 256, 512, 1024, 2048)
    assert bb.encoder_layout(name) == (4, LAYERS[name])
    assert bb.encoder_groups(name) == WIDTHS[name] and bb.encoder_groups("resnet50") == (1, 64) and bb.encoder_groups("resnet18") == (1, 64)
    groups, wpg = WIDTHS[name]
    for L, n in enumerate(LAYERS[name]):
        layer = getattr(enc, f"layer{L + 1}")
        assert len(layer) == n
        cg = 64 * 2 ** L * wpg // 64
        for blk in layer:
            assert tuple(blk.conv2.weight.shape) == (cg * groups, cg, 3, 3) and blk.conv2.groups == groups
            assert blk.conv1.out_channels == cg * groups and blk.conv3.in_channels == cg * groups
            assert blk.conv3.out_channels == 256 * 2 ** L


def test_unbuilt_variants_raise_keyerror_with_the_new_names():
    from fastposecnn_amd.lib import backbone as bb
    for name in ("resnext101_32x16d", "resnext101_32x32d", "resnext101_32x48d", "se_resnext50_32x4d"):
        with pytest.raises(KeyError) as e:
            bb.get_encoder(name)
        assert "resnext50_32x4d" in str(e.value)


def test_stride_on_conv2_and_downsample_on_block0_only():
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder("resnext50_32x4d")
    for L in range(1, 5):
        layer = getattr(enc, f"layer{L}")
        s = 1 if L == 1 else 2
        assert layer[0].conv1.stride == (1, 1) and layer[0].conv1.kernel_size == (1, 1)
        assert layer[0].conv2.stride == (s, s) and layer[0].conv2.kernel_size == (3, 3) and layer[0].conv2.padding == (1, 1)
        assert all(blk.conv2.stride == (1, 1) for blk in layer[1:])
        assert layer[0].downsample is not None and layer[0].downsample[0].stride == (s, s)
        assert all(blk.downsample is None for blk in layer[1:])
        assert all(isinstance(c, bb.Conv2d) for blk in layer for c in (blk.conv1, blk.conv2, blk.conv3))


def test_state_dict_names_equal_resnet50s_and_cpu_forward():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(0)
    enc = bb.get_encoder("resnext50_32x4d").eval()
    assert list(enc.state_dict()) == list(bb.get_encoder("resnet50").state_dict())
    with torch.no_grad():
        feats = enc(torch.randn(1, 3, 64, 96))
    assert [tuple(f.shape) for f in feats] == [(1, 3, 64, 96), (1, 64, 32, 48), (1, 256, 16, 24), (1, 512, 8, 12),
                                                (1, 1024, 4, 6), (1, 2048, 2, 3)]
    assert all(torch.isfinite(f).all() for f in feats)


def test_grouped_conv2d_module_is_torchs_grouped_convolution():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(1)
    c = bb.Conv2d(64, 64, 3, 2, 1, groups=16, bias=False).train()
    x = torch.randn(2, 64, 9, 11)
    assert torch.equal(c(x), torch.nn.functional.conv2d(x, c.weight, None, 2, 1, 1, 16))


def test_load_from_ckpt_resnext50_round_trip(tmp_path):
    """A Lightning-style checkpoint whose hyper-parameters name the ResNeXt-50 encoder loads (KeyError before)."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config, synth
    hp_src = config.HEAD_TRAINING()
    hp_src.ENCODER = 'resnext50_32x4d'
    torch.manual_seed(5)
    src = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp_src).eval()
    ckpt = {'state_dict': {'model.' + k: v.clone() for k, v in src.state_dict().items()},
            'hyper_parameters': {'MODEL': 'PoseRegressor', 'BACKBONE_ARCH': 'FPN', 'ENCODER': 'resnext50_32x4d',
                                 'ENCODER_WEIGHTS': None, 'SELECTED_CLASSES': hp_src.SELECTED_CLASSES}}
    path = tmp_path / "last.ckpt"
    torch.save(ckpt, path)
    hp = config.INFERENCE()
    torch.manual_seed(77)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(str(path), hp).eval()
    assert hp.ENCODER == 'resnext50_32x4d' and m.encoder.name == 'resnext50_32x4d'
    sd, want = m.state_dict(), src.state_dict()
    assert list(sd) == list(want)
    for k in want:
        assert torch.equal(sd[k], want[k]), k
    x = synth.make_image(0, 64, 64)[None]
    hp.PERFORM_AGGREGATION = False
    hp_src.PERFORM_AGGREGATION = False
    with torch.no_grad():
        a, b = m(x), src(x)
    for k in a["logits"]:
        assert torch.equal(a["logits"][k], b["logits"][k]), k


def test_encoder_weights_file_with_torchvision_keys(tmp_path, monkeypatch):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(4)
    donor = bb.ResNetEncoder('resnext50_32x4d')
    tv = {k: v.clone() for k, v in donor.state_dict().items()}
    tv['fc.weight'] = torch.zeros(1000, 2048); tv['fc.bias'] = torch.zeros(1000)
    f = tmp_path / "rx50.pth"
    torch.save(tv, f)
    monkeypatch.setenv("FPC_ENCODER_WEIGHTS", str(f))
    torch.manual_seed(8)
    enc = bb.get_encoder('resnext50_32x4d', weights='imagenet')
    assert enc.loaded_weights == str(f)
    assert all(torch.equal(v, donor.state_dict()[k]) for k, v in enc.state_dict().items())
    with pytest.raises(RuntimeError):
        bb.get_encoder('resnet50', weights='imagenet')          # a ResNeXt file is not a ResNet-50 file: strict loading


def test_preprocessing_params_answer_the_resnext_names():
    from fastposecnn_amd.tools import dataset
    assert dataset.get_preprocessing_params("resnext50_32x4d") == dataset.get_preprocessing_params("resnet50")


def _create_ex(hiplib, block, layers, groups, width, classes=7, B=2, H=480, W=640):
    h = ctypes.c_void_p()
    rc = hiplib.fpc_net_create_encoder_ex(block, (ctypes.c_int * 4)(*layers), groups, width, classes, B, H, W, ctypes.byref(h))
    return rc, h


def _plans(hiplib, h):
    out = (ctypes.c_int * 5)()
    res = []
    for i in range(hiplib.fpc_net_conv_count(h)):
        assert hiplib.fpc_net_conv_plan(h, i, out) == 0
        res.append(tuple(out))
    return res


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_engine_param_table_matches_state_dict(hiplib, name):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = name
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    rc, h = _create_ex(hiplib, 4, LAYERS[name], *WIDTHS[name])
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
        assert hiplib.fpc_net_param_count(g) == n and hiplib.fpc_net_workspace_bytes(g) == hiplib.fpc_net_workspace_bytes(h) > 0
        assert hiplib.fpc_net_forward(h, *([None] * 11), None) == -1       # before load_params: refused, not a crash
        # the grouped code at exactly the conv2 sites: K = 9 Cg there, and the site's width is groups x Cg
        plans = _plans(hiplib, h)
        assert plans == _plans(hiplib, g)
        grouped = [p for p in plans if FPC_PLAN_GROUPED <= p[2] < FPC_PLAN_GROUPED + 1000]
        assert len(grouped) == sum(LAYERS[name]) == {"resnext50_32x4d": 16}.get(name, 33)
        groups, wpg = WIDTHS[name]
        want = [(64 * 2 ** L * wpg // 64) for L, cnt in enumerate(LAYERS[name]) for _ in range(cnt)]
        assert [p[4] for p in grouped] == [9 * cg for cg in want]
        assert [p[3] for p in grouped] == [groups * cg for cg in want]
        assert all(p[2] == FPC_PLAN_GROUPED and p[1] == 32 for p in grouped)
    finally:
        hiplib.fpc_net_destroy(h)
        hiplib.fpc_net_destroy(g)


@pytest.mark.parametrize("layers", [[3, 4, 6, 3], [3, 4, 23, 3], [1, 1, 1, 1]])
def test_ex_descriptor_without_groups_equals_the_plain_one(hiplib, layers):
    for B, H, W in ((1, 480, 640), (32, 480, 640), (2, 64, 96)):
        rc, h = _create_ex(hiplib, 4, layers, 1, 64, B=B, H=H, W=W)
        assert rc == 0
        g = ctypes.c_void_p()
        assert hiplib.fpc_net_create_encoder(4, (ctypes.c_int * 4)(*layers), 7, B, H, W, ctypes.byref(g)) == 0
        try:
            n = hiplib.fpc_net_param_count(h)
            assert n == hiplib.fpc_net_param_count(g)
            for i in range(n):
                assert hiplib.fpc_net_param_name(h, i) == hiplib.fpc_net_param_name(g, i)
                assert hiplib.fpc_net_param_numel(h, i) == hiplib.fpc_net_param_numel(g, i)
            assert hiplib.fpc_net_workspace_bytes(h) == hiplib.fpc_net_workspace_bytes(g)
            assert _plans(hiplib, h) == _plans(hiplib, g)
            assert not any(p[2] >= FPC_PLAN_GROUPED for p in _plans(hiplib, h))
        finally:
            hiplib.fpc_net_destroy(h)
            hiplib.fpc_net_destroy(g)
    rc, h = _create_ex(hiplib, 1, [2, 2, 2, 2], 1, 64)       # BasicBlock through the same entry
    assert rc == 0
    hiplib.fpc_net_destroy(h)


def test_refusals(hiplib):
    R50 = [3, 4, 6, 3]
    for block, groups, width in ((1, 32, 4),      # groups on BasicBlock
                                 (4, 32, 3),      # 3 / 6 / 12 / 24 channels per group
                                 (4, 32, 16),     # 128 channels per group at layer4
                                 (4, 32, 1),      # 1 .. 8
                                 (4, 1, 128),     # a wide ResNet: no groups, another width
                                 (4, 0, 64), (4, -32, 4), (4, 32, 0)):
        rc, _ = _create_ex(hiplib, block, R50, groups, width)
        assert rc == -1, (block, groups, width)
    h = ctypes.c_void_p()
    assert hiplib.fpc_net_create_encoder_ex(4, None, 32, 4, 7, 1, 480, 640, ctypes.byref(h)) == -1
    rc, _ = _create_ex(hiplib, 4, R50, 32, 4, H=481)
    assert rc == -1
    for name in (b"resnext101_32x16d", b"resnext50", b"resnet50"):       # names the named entry point does not answer
        assert hiplib.fpc_net_create(name, 7, 1, 480, 640, ctypes.byref(h)) == -1
    # the stand-alone entry's workspace: 0 for what it refuses
    assert hiplib.fpc_conv2d_grouped_workspace_bytes(128, 32) >= 128 * 4 * 9 * 4
    for C, groups in ((128, 24), (128, 64), (128, 1), (48, 12), (128, 0)):
        assert hiplib.fpc_conv2d_grouped_workspace_bytes(C, groups) == 0, (C, groups)


def test_abi_version_is_unchanged(hiplib):
    assert hiplib.fpc_abi_version() == 11
