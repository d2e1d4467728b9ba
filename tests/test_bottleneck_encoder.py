"""CPU checks of the Bottleneck encoders (ResNet-50 / 101 / 152): the module restatement against torchvision's shapes and
names, checkpoint and encoder-weights loading, and the engine's host-side plan (fpc_net_create_encoder: parameter table,
refused descriptors) and the 1x1 GEMM's request code in the stand-alone convolution's planner.  No compute calls into the
HIP library."""
import ctypes

import pytest
import torch

# torchvision's totals minus the 2 049 000 parameters of `fc`
PARAMS = {"resnet50": 23_508_032, "resnet101": 42_500_160, "resnet152": 58_143_808}
LAYERS = {"resnet50": [3, 4, 6, 3], "resnet101": [3, 4, 23, 3], "resnet152": [3, 8, 36, 3]}


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_encoder_parameter_count_and_channels(name):
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder(name)
    assert sum(p.numel() for p in enc.parameters()) == PARAMS[name]
    assert enc.out_channels == (3, 64, 256, 512, 1024, 2048)
    assert bb.encoder_layout(name) == (4, LAYERS[name])
    for L, n in enumerate(LAYERS[name]):
        assert len(getattr(enc, f"layer{L + 1}")) == n


def test_fpn_decoder_over_bottleneck_widths():
    from fastposecnn_amd.lib import backbone as bb
    dec = bb.FPNDecoder((3, 64, 256, 512, 1024, 2048))
    assert sum(p.numel() for p in dec.parameters()) == 2_607_872


def test_stride_on_conv2_and_downsample_on_block0_only():
    from fastposecnn_amd.lib import backbone as bb
    enc = bb.get_encoder("resnet50")
    for L in range(1, 5):
        layer = getattr(enc, f"layer{L}")
        s = 1 if L == 1 else 2
        assert layer[0].conv1.stride == (1, 1) and layer[0].conv1.kernel_size == (1, 1)
        assert layer[0].conv2.stride == (s, s) and layer[0].conv2.kernel_size == (3, 3)
        assert layer[0].conv3.kernel_size == (1, 1) and layer[0].conv3.out_channels == 4 * layer[0].conv1.out_channels
        assert layer[0].downsample is not None and layer[0].downsample[0].stride == (s, s)      # layer1 too: 64 != 256
        assert all(blk.downsample is None for blk in layer[1:])
        assert all(isinstance(c, bb.Conv2d) for blk in layer for c in (blk.conv1, blk.conv2, blk.conv3))


def test_state_dict_names_and_cpu_forward():
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = "resnet50"
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).eval()
    sd = m.state_dict()
    for k in ("encoder.layer4.2.bn3.running_var", "encoder.layer1.0.downsample.0.weight", "encoder.layer1.0.downsample.1.bias",
              "encoder.layer3.5.conv3.weight", "mask_decoder.p5.weight", "mask_decoder.p2.skip_conv.weight"):
        assert k in sd, k
    assert "encoder.layer1.1.downsample.0.weight" not in sd and not any(k.startswith("encoder.fc.") for k in sd)
    assert tuple(sd["mask_decoder.p5.weight"].shape) == (256, 2048, 1, 1)
    assert tuple(sd["mask_decoder.p2.skip_conv.weight"].shape) == (256, 256, 1, 1)
    with torch.no_grad():
        feats = m.encoder(torch.zeros(1, 3, 64, 96))
    assert [tuple(f.shape) for f in feats] == [(1, 3, 64, 96), (1, 64, 32, 48), (1, 256, 16, 24), (1, 512, 8, 12),
                                                (1, 1024, 4, 6), (1, 2048, 2, 3)]


def test_load_from_ckpt_resnet50_round_trip(tmp_path):
    """A Lightning-style checkpoint whose hyper-parameters name a ResNet-50 encoder loads (it raised KeyError before)."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config, synth
    hp_src = config.HEAD_TRAINING()
    hp_src.ENCODER = 'resnet50'
    torch.manual_seed(5)
    src = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp_src).eval()
    ckpt = {'state_dict': {'model.' + k: v.clone() for k, v in src.state_dict().items()},
            'hyper_parameters': {'MODEL': 'PoseRegressor', 'BACKBONE_ARCH': 'FPN', 'ENCODER': 'resnet50',
                                 'ENCODER_WEIGHTS': None, 'SELECTED_CLASSES': hp_src.SELECTED_CLASSES}}
    path = tmp_path / "last.ckpt"
    torch.save(ckpt, path)
    hp = config.INFERENCE()
    torch.manual_seed(77)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(str(path), hp).eval()
    assert hp.ENCODER == 'resnet50' and m.encoder.name == 'resnet50'
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
    import backbone as bb
    torch.manual_seed(4)
    donor = bb.ResNetEncoder('resnet50')
    tv = {k: v.clone() for k, v in donor.state_dict().items()}
    tv['fc.weight'] = torch.zeros(1000, 2048); tv['fc.bias'] = torch.zeros(1000)
    f = tmp_path / "r50.pth"
    torch.save(tv, f)
    monkeypatch.setenv("FPC_ENCODER_WEIGHTS", str(f))
    torch.manual_seed(8)
    enc = bb.get_encoder('resnet50', weights='imagenet')
    assert enc.loaded_weights == str(f)
    assert all(torch.equal(v, donor.state_dict()[k]) for k, v in enc.state_dict().items())


def _create(hiplib, block, layers, classes=7, B=2, H=480, W=640):
    h = ctypes.c_void_p()
    rc = hiplib.fpc_net_create_encoder(block, (ctypes.c_int * 4)(*layers), classes, B, H, W, ctypes.byref(h))
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
    rc, h = _create(hiplib, 4, LAYERS[name])
    assert rc == 0
    try:
        n = hiplib.fpc_net_param_count(h)
        names = [hiplib.fpc_net_param_name(h, i).decode() for i in range(n)]
        assert len(set(names)) == n
        for i, nm in enumerate(names):
            assert nm in sd, nm
            assert sd[nm].numel() == hiplib.fpc_net_param_numel(h, i), nm
        unused = [k for k in sd if k not in set(names) and not k.endswith("num_batches_tracked")]
        assert unused == []
        assert hiplib.fpc_net_workspace_bytes(h) > 0
        assert hiplib.fpc_net_forward(h, *([None] * 11), None) == -1       # before load_params: refused, not a crash
        out = (ctypes.c_int * 5)()
        for i in range(hiplib.fpc_net_conv_count(h)):
            assert hiplib.fpc_net_conv_plan(h, i, out) == 0
    finally:
        hiplib.fpc_net_destroy(h)


@pytest.mark.parametrize("name,layers", [("resnet18", [2, 2, 2, 2]), ("resnet34", [3, 4, 6, 3])])
def test_basic_block_descriptor_equals_the_named_net(hiplib, name, layers):
    for B, H, W in ((1, 480, 640), (32, 480, 640), (2, 64, 96)):
        rc, h = _create(hiplib, 1, layers, B=B, H=H, W=W)
        assert rc == 0
        g = ctypes.c_void_p()
        assert hiplib.fpc_net_create(name.encode(), 7, B, H, W, ctypes.byref(g)) == 0
        try:
            n = hiplib.fpc_net_param_count(h)
            assert n == hiplib.fpc_net_param_count(g)
            for i in range(n):
                assert hiplib.fpc_net_param_name(h, i) == hiplib.fpc_net_param_name(g, i)
                assert hiplib.fpc_net_param_numel(h, i) == hiplib.fpc_net_param_numel(g, i)
            assert hiplib.fpc_net_workspace_bytes(h) == hiplib.fpc_net_workspace_bytes(g)
            a, b = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
            assert hiplib.fpc_net_conv_count(h) == hiplib.fpc_net_conv_count(g)
            for i in range(hiplib.fpc_net_conv_count(h)):
                hiplib.fpc_net_conv_plan(h, i, a)
                hiplib.fpc_net_conv_plan(g, i, b)
                assert tuple(a) == tuple(b)
        finally:
            hiplib.fpc_net_destroy(h)
            hiplib.fpc_net_destroy(g)


def test_bad_descriptors_are_refused(hiplib):
    h = ctypes.c_void_p()
    for block, layers, kw in ((2, [3, 4, 6, 3], {}), (0, [3, 4, 6, 3], {}), (4, [3, 0, 6, 3], {}), (4, [3, 4, 6, -1], {}),
                              (4, [3, 4, 6, 3], dict(H=481)), (4, [3, 4, 6, 3], dict(W=100)), (4, [3, 4, 6, 3], dict(classes=1)),
                              (4, [3, 4, 6, 3], dict(B=0))):
        rc, _ = _create(hiplib, block, layers, **kw)
        assert rc == -1, (block, layers, kw)
    assert hiplib.fpc_net_create_encoder(4, None, 7, 1, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_force_pointwise(None, 1) == -1
    assert hiplib.fpc_net_create(b"resnet50", 7, 1, 480, 640, ctypes.byref(h)) == -1       # the named entry point is unchanged


def test_force_pointwise_counts_the_1x1_sites_host_only(hiplib):
    """Plans only (no forward): every 1x1 site moves to the new form and back; 3x3 sites and the stem never move."""
    rc, h = _create(hiplib, 4, [3, 4, 6, 3], B=1)
    assert rc == 0
    try:
        out = (ctypes.c_int * 5)()
        n = hiplib.fpc_net_conv_count(h)
        before = []
        for i in range(n):
            hiplib.fpc_net_conv_plan(h, i, out)
            before.append(tuple(out))
        # encoder: 16 conv1 + 16 conv3 + 4 downsample; decoders: the 4 lateral levels, one grouped site each
        assert hiplib.fpc_net_force_pointwise(h, 1) == 36 + 4
        assert hiplib.fpc_net_force_pointwise(h, 1) == 0
        moved = 0
        for i in range(n):
            hiplib.fpc_net_conv_plan(h, i, out)
            if out[2] == 4000:
                moved += 1
                assert out[0] == 64 and out[1] == 64
        assert moved == 40
        assert hiplib.fpc_net_force_pointwise(h, 0) == 40
        for i in range(n):
            hiplib.fpc_net_conv_plan(h, i, out)
            assert tuple(out) == before[i], i
        assert hiplib.fpc_net_force_pointwise(h, 2) == -1
    finally:
        hiplib.fpc_net_destroy(h)


def test_workspace_of_the_bottleneck_nets(hiplib):
    """Workspace bytes at B = 32, 640 x 480 (DESIGN.md states them): deeper nets differ by their weights only, since a stage's
    blocks share their activation buffers."""
    ws = {}
    for name in ("resnet50", "resnet101", "resnet152"):
        rc, h = _create(hiplib, 4, LAYERS[name], B=32)
        assert rc == 0
        ws[name] = hiplib.fpc_net_workspace_bytes(h)
        hiplib.fpc_net_destroy(h)
    assert ws["resnet50"] < ws["resnet101"] < ws["resnet152"]
    assert ws["resnet152"] - ws["resnet50"] < 2 * 10 * 4 * (PARAMS["resnet152"] - PARAMS["resnet50"])      # weights, not activations


@pytest.mark.parametrize("variant", [0, 1])
def test_conv2d_plan_accepts_the_pointwise_code(hiplib, variant):
    out = (ctypes.c_int * 4)()
    for B, Ho, Wo, Cin, Cout in ((1, 15, 20, 2048, 512), (32, 120, 160, 64, 256), (3, 7, 9, 256, 64)):
        assert hiplib.fpc_conv2d_plan(B, Ho, Wo, Cin, Cout, 1, 1, 0, 0, 4000 + variant, out) == 0
        assert out[2] == 1                                     # no split over K
        nb = hiplib.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, Cin, Cout, 1, 1, 0, 0, 4000 + variant)
        assert 2.5 * 4 * Cin * Cout <= nb <= hiplib.fpc_conv2d_workspace_bytes(B, Ho, Wo, Cin, Cout, 1, 1)
