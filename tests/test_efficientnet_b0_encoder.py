"""CPU checks of the EfficientNet-B0 encoder (efficientnet-b0): the module restatement against the published definition of
efficientnet_pytorch's EfficientNet as smp's EfficientNetEncoder wraps it (parameter counts by plain arithmetic, state-dict names
against a committed manifest, feature levels, BatchNorm constants, the static pads, the block formula in float64), checkpoint and
encoder-weights loading, the preprocessing parameters, the engine's host-side plan (fpc_net_create("efficientnet-b0"): parameter
table, refusals) and the host-side refusals of the stand-alone kernel entries.  No compute calls into the HIP library."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "efficientnet-b0"
# (repeat, kernel, stride, expand ratio, input, output)
BLOCKS = [(1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80), (3, 5, 1, 6, 80, 112),
          (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)]
# the 16 blocks as (k, stride, Cin, Ce, Cs, Cout, skip)
TABLE = [(3, 1, 32, 32, 8, 16, False), (3, 2, 16, 96, 4, 24, False), (3, 1, 24, 144, 6, 24, True), (5, 2, 24, 144, 6, 40, False),
         (5, 1, 40, 240, 10, 40, True), (3, 2, 40, 240, 10, 80, False), (3, 1, 80, 480, 20, 80, True), (3, 1, 80, 480, 20, 80, True),
         (5, 1, 80, 480, 20, 112, False), (5, 1, 112, 672, 28, 112, True), (5, 1, 112, 672, 28, 112, True),
         (5, 2, 112, 672, 28, 192, False), (5, 1, 192, 1152, 48, 192, True), (5, 1, 192, 1152, 48, 192, True),
         (5, 1, 192, 1152, 48, 192, True), (3, 1, 192, 1152, 48, 320, False)]
PARAMS_RUN, PARAMS_ALL = 3_595_388, 4_007_548


def table_from_block_args():
    out = []
    for repeat, k, stride, expand, cin, cout in BLOCKS:
        for i in range(repeat):
            inp = cin if i == 0 else cout
            s = stride if i == 0 else 1
            out.append((k, s, inp, inp * expand, max(1, int(inp * 0.25)), cout, s == 1 and inp == cout))
    return out


def params_by_arithmetic():
    """Weights, biases and BatchNorm affines of what the forward runs, and with _conv_head / _bn1."""
    total = 32 * 3 * 9 + 2 * 32
    for k, _, cin, ce, cs, cout, _ in TABLE:
        if ce != cin:
            total += ce * cin + 2 * ce
        total += ce * k * k + 2 * ce + (cs * ce + cs) + (ce * cs + ce) + cout * ce + 2 * cout
    return total, total + 1280 * 320 + 2 * 1280


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


@pytest.fixture(scope="module")
def enc():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(0)
    return bb.get_encoder(NAME)


def test_parameter_counts(enc):
    assert table_from_block_args() == TABLE
    assert params_by_arithmetic() == (PARAMS_RUN, PARAMS_ALL)
    assert sum(p.numel() for p in enc.parameters()) == PARAMS_ALL
    idle = ("_conv_head.", "_bn1.")
    assert sum(p.numel() for n, p in enc.named_parameters() if not n.startswith(idle)) == PARAMS_RUN


def test_state_dict_key_order_equals_the_manifest(enc):
    """The manifest is written by tests/golden/make_state_dict_keys_efficientnet_b0.py from the published definition, not dumped from
    this module."""
    want = open(os.path.join(HERE, "golden", "state_dict_keys_efficientnet_b0.txt")).read().split()
    assert len(want) == 358
    assert list(enc.state_dict()) == want
    assert not any(k.startswith("_fc") for k in want) and want[-6] == "_conv_head.weight" and want[-1] == "_bn1.num_batches_tracked"
    sd = enc.state_dict()
    assert tuple(sd["_conv_stem.weight"].shape) == (32, 3, 3, 3) and tuple(sd["_conv_head.weight"].shape) == (1280, 320, 1, 1)
    for i, (k, _, cin, ce, cs, cout, _) in enumerate(TABLE):
        p = f"_blocks.{i}."
        assert (p + "_expand_conv.weight" in sd) == (ce != cin) == (p + "_bn0.weight" in sd)
        assert tuple(sd[p + "_depthwise_conv.weight"].shape) == (ce, 1, k, k)
        assert tuple(sd[p + "_se_reduce.weight"].shape) == (cs, ce, 1, 1) and tuple(sd[p + "_se_reduce.bias"].shape) == (cs,)
        assert tuple(sd[p + "_se_expand.weight"].shape) == (ce, cs, 1, 1) and tuple(sd[p + "_se_expand.bias"].shape) == (ce,)
        assert tuple(sd[p + "_project_conv.weight"].shape) == (cout, ce, 1, 1)
    biased = [k for k in want if k.endswith("conv.bias") or k.endswith("_se_reduce.bias") or k.endswith("_se_expand.bias")]
    assert len(biased) == 32 and all("_se_" in k for k in biased)


def test_module_properties(enc):
    from fastposecnn_amd.lib import backbone as bb
    assert isinstance(enc, bb.EfficientNetEncoder) and enc.name == NAME
    assert enc.out_channels == (3, 32, 24, 40, 112, 320) and enc.drop_connect_rate == 0.2
    assert bb.encoder_family(NAME) == "efficientnet" and bb.encoder_family("mobilenet_v2") == "mobilenet_v2"
    assert bb.encoder_family("resnet18") == "resnet"
    for other in ("efficientnet-b1", "efficientnet_b0", "efficientnet"):
        with pytest.raises(KeyError):
            bb.encoder_family(other)
        with pytest.raises(KeyError, match="efficientnet-b0"):      # the message lists what there is
            bb.get_encoder(other)
    assert not hasattr(enc, "_fc") and len(enc._blocks) == 16
    with torch.no_grad():
        feats = enc.eval()(torch.randn(1, 3, 64, 96))
    assert [tuple(f.shape[1:]) for f in feats] == [(3, 64, 96), (32, 32, 48), (24, 16, 24), (40, 8, 12), (112, 4, 6), (320, 2, 3)]
    assert all(torch.isfinite(f).all() for f in feats)
    bns = [m for m in enc.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 1 + 15 + 16 + 16 + 1
    assert all(isinstance(m, bb.BatchNorm2d) and m.eps == 1e-3 and m.momentum == 0.01 for m in bns)
    for blk, (k, s, cin, ce, cs, cout, skip) in zip(enc._blocks, TABLE):
        dw = blk._depthwise_conv
        assert dw.kernel_size == (k, k) and dw.stride == (s, s) and dw.groups == ce == dw.in_channels and dw.padding == (0, 0)
        assert blk.use_skip == skip and blk._se_reduce.out_channels == cs and blk._project_conv.out_channels == cout
        # the static pads, (left, right, top, bottom): fixed numbers that do not depend on the input
        before = (k - 1) // 2 if s == 1 else (k - 3) // 2
        after = (k - 1) // 2 if s == 1 else k - 2 - before
        assert isinstance(dw.static_padding, torch.nn.ZeroPad2d) and tuple(dw.static_padding.padding) == (before, after, before, after)
        assert isinstance(blk._project_conv.static_padding, torch.nn.Identity)
    assert tuple(enc._conv_stem.static_padding.padding) == (0, 1, 0, 1) and enc._conv_stem.stride == (2, 2)
    assert [i for i, b in enumerate(enc._blocks) if b.stride == 2] == [1, 3, 5, 11]


def _swish(v):
    return v * torch.sigmoid(v)


def _bn(v, bn):
    sh = (1, -1, 1, 1)
    return (v - bn.running_mean.view(sh)) / torch.sqrt(bn.running_var.view(sh) + 1e-3) * bn.weight.view(sh) + bn.bias.view(sh)


@pytest.mark.parametrize("idx", [0, 2, 3, 15], ids=["no-expand", "skip-k3", "k5-stride2", "last"])
def test_block_forward_is_the_published_formula(idx):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(3)
    e = bb.get_encoder(NAME)
    g = torch.Generator().manual_seed(idx)
    for m in e.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    k, s, cin, ce, cs, cout, skip = TABLE[idx]
    blk = e._blocks[idx].eval().double()
    x = torch.randn(2, cin, 6, 10, dtype=torch.float64) * 3.0
    # the pads by the table of the definition: stride 1 (k - 1) / 2 on every side; stride 2 pads 0 / 1 for k = 3 and 1 / 2 for k = 5
    lo, hi = {(3, 1): (1, 1), (5, 1): (2, 2), (3, 2): (0, 1), (5, 2): (1, 2)}[(k, s)]
    with torch.no_grad():
        v = x
        if idx != 0:
            v = _swish(_bn(F.conv2d(v, blk._expand_conv.weight), blk._bn0))
        assert v.shape[1] == ce
        v = _swish(_bn(F.conv2d(F.pad(v, (lo, hi, lo, hi)), blk._depthwise_conv.weight, None, s, 0, 1, ce), blk._bn1))
        gate = F.conv2d(v.mean(dim=(2, 3), keepdim=True), blk._se_reduce.weight, blk._se_reduce.bias)
        gate = torch.sigmoid(F.conv2d(_swish(gate), blk._se_expand.weight, blk._se_expand.bias))
        assert tuple(gate.shape) == (2, ce, 1, 1)
        want = _bn(F.conv2d(v * gate, blk._project_conv.weight), blk._bn2)
        if skip:
            want = want + x
        got = blk(x)
        blk.train()
        blk.drop_connect_rate = 0.0                               # training mode without drop-connect: batch statistics only
        assert blk(x).shape == got.shape
    assert tuple(got.shape) == (2, cout, 6 // s, 10 // s)
    assert (got < 0).any()                                         # no activation behind the projection / the add
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_drop_connect_runs_in_training_only():
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(1)
    e = bb.get_encoder(NAME)
    x = torch.randn(8, 3, 32, 32)
    e.train()
    with torch.no_grad():
        e(x)
    assert [b.drop_connect_rate for b in e._blocks] == [0.2 * i / 16 for i in range(16)]
    blk = e._blocks[2]
    xb = torch.randn(64, 24, 4, 4)
    blk.drop_connect_rate = 0.5
    with torch.no_grad():
        y = blk(xb) - xb                                           # the branch: zero for a dropped frame, scaled by 2 for a kept one
    dropped = (y.abs().amax(dim=(1, 2, 3)) == 0).sum().item()
    assert 0 < dropped < 64
    blk.eval()
    with torch.no_grad():
        assert ((blk(xb) - xb).abs().amax(dim=(1, 2, 3)) > 0).all()


def test_load_from_ckpt_round_trip(tmp_path):
    """A Lightning-style checkpoint whose hyper-parameters name efficientnet-b0 loads (KeyError before) and reproduces the donor's
    logits bit for bit."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config, synth
    hp_src = config.HEAD_TRAINING()
    hp_src.ENCODER = NAME
    torch.manual_seed(5)
    src = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp_src).eval()
    ckpt = {'state_dict': {'model.' + k: v.clone() for k, v in src.state_dict().items()},
            'hyper_parameters': {'MODEL': 'PoseRegressor', 'BACKBONE_ARCH': 'FPN', 'ENCODER': NAME,
                                 'ENCODER_WEIGHTS': None, 'SELECTED_CLASSES': hp_src.SELECTED_CLASSES}}
    path = tmp_path / "last.ckpt"
    torch.save(ckpt, path)
    hp = config.INFERENCE()
    torch.manual_seed(77)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(str(path), hp).eval()
    assert hp.ENCODER == NAME and m.encoder.name == NAME
    sd, want = m.state_dict(), src.state_dict()
    assert list(sd) == list(want)
    assert "encoder._conv_stem.weight" in sd and "encoder._blocks.3._bn1.running_var" in sd and "encoder._conv_head.weight" in sd
    assert tuple(sd["mask_decoder.p2.skip_conv.weight"].shape) == (256, 24, 1, 1)
    assert tuple(sd["mask_decoder.p5.weight"].shape) == (256, 320, 1, 1)
    for k in want:
        assert torch.equal(sd[k], want[k]), k
    x = synth.make_image(0, 64, 64)[None]
    hp.PERFORM_AGGREGATION = False
    hp_src.PERFORM_AGGREGATION = False
    with torch.no_grad():
        a, b = m(x), src(x)
    for k in a["logits"]:
        assert torch.equal(a["logits"][k], b["logits"][k]), k


def test_encoder_weights_file_with_fc(tmp_path, monkeypatch):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(4)
    donor = bb.EfficientNetEncoder()
    full = {k: v.clone() for k, v in donor.state_dict().items()}
    full['_fc.weight'] = torch.zeros(1000, 1280); full['_fc.bias'] = torch.zeros(1000)
    f = tmp_path / "efficientnet-b0.pth"
    torch.save(full, f)
    monkeypatch.setenv("FPC_ENCODER_WEIGHTS", str(f))
    torch.manual_seed(8)
    enc = bb.get_encoder(NAME, weights='imagenet')
    assert enc.loaded_weights == str(f)
    assert all(torch.equal(v, donor.state_dict()[k]) for k, v in enc.state_dict().items())
    assert "_conv_head.weight" in enc.state_dict()                  # kept, as smp keeps it
    with pytest.raises(RuntimeError):
        bb.get_encoder('mobilenet_v2', weights='imagenet')          # strict loading: another encoder's file is refused
    del full['_conv_head.weight']
    torch.save(full, f)
    with pytest.raises(RuntimeError):
        bb.get_encoder(NAME, weights='imagenet')                    # ... and a file without the head is not a full state dict


def test_preprocessing_params_answer_the_name():
    from fastposecnn_amd.tools import dataset
    assert dataset.get_preprocessing_params(NAME) == dataset.get_preprocessing_params("resnet18")
    assert dataset.get_preprocessing_params(NAME)["mean"] == [0.485, 0.456, 0.406]
    with pytest.raises(ValueError):
        dataset.get_preprocessing_params("efficientnet-b1")


def test_engine_param_table_matches_state_dict(hiplib):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = NAME
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    h = ctypes.c_void_p()
    assert hiplib.fpc_net_create(NAME.encode(), 7, 2, 480, 640, ctypes.byref(h)) == 0
    try:
        n = hiplib.fpc_net_param_count(h)
        names = [hiplib.fpc_net_param_name(h, i).decode() for i in range(n)]
        assert len(set(names)) == n
        for i, nm in enumerate(names):
            assert nm in sd, nm
            assert sd[nm].numel() == hiplib.fpc_net_param_numel(h, i), nm
        idle = ("encoder._conv_head.", "encoder._bn1.")              # in the state_dict, not run, not in the table
        unused = [k for k in sd if k not in set(names) and not k.endswith("num_batches_tracked")]
        assert unused == ["encoder._conv_head.weight", "encoder._bn1.weight", "encoder._bn1.bias", "encoder._bn1.running_mean",
                          "encoder._bn1.running_var"]
        order = [k for k in m.state_dict() if k.startswith("encoder.") and not k.endswith("num_batches_tracked") and not k.startswith(idle)]
        assert [nm for nm in names if nm.startswith("encoder.")] == order and len(order) == 48 * 5 + 16 * 4
        assert sum(hiplib.fpc_net_param_numel(h, i) for i, nm in enumerate(names)
                   if nm.startswith("encoder.") and not nm.endswith(("running_mean", "running_var"))) == PARAMS_RUN
        assert names.index("mask_decoder.p5.weight") == len(order)         # then the decoders and heads, as on every plan
        assert hiplib.fpc_net_workspace_bytes(h) > 0
        assert hiplib.fpc_net_forward(h, *([None] * 11), None) == -1          # before load_params: refused, not a crash
        assert hiplib.fpc_net_force_stem_pool(h, 1) == -1 and hiplib.fpc_net_force_stem_pool(h, 0) == -1
        assert hiplib.fpc_net_force_fold(h, 1) == -1 and hiplib.fpc_net_force_fold(h, 0) == 0
        # the convolution sites are the decoders' alone: 4 x (4 laterals + 7 segmentation convolutions); the laterals read 320 / 112 /
        # 40 / 24 channels
        out = (ctypes.c_int * 5)()
        plans = []
        for i in range(hiplib.fpc_net_conv_count(h)):
            assert hiplib.fpc_net_conv_plan(h, i, out) == 0
            plans.append(tuple(out))
        assert len(plans) == 44
        assert [p[4] for p in plans[:4]] == [320, 112, 40, 24] and all(p[3] == 256 for p in plans[:4])
        # FLOP of a frame: the encoder's 48 convolutions by arithmetic (2.23 G multiply-adds at 640 x 480: the published 0.39 G at 224 x 224
        # scaled by the pixels, less _conv_head's 0.12 G; the gate's two tiny layers are not counted) + what the decoder sites and heads count
        fl = (ctypes.c_double * 3)()
        assert hiplib.fpc_net_flops(h, fl) == 0
        hw = 240 * 320
        enc_macs = hw * 32 * 27
        for k, s, cin, ce, cs, cout, _ in TABLE:
            if ce != cin:
                enc_macs += hw * cin * ce
            hw //= s * s
            enc_macs += hw * ce * k * k + hw * ce * cout
        assert hw == 15 * 20 and 2.2e9 < enc_macs < 2.25e9 and 0.38e9 < (enc_macs + 300 * 320 * 1280) * 224 * 224 / (640 * 480) < 0.40e9
        dec = sum(2.0 * 2 * hwl * 256 * cin * 4 for hwl, cin in ((300, 320), (1200, 112), (4800, 40), (19200, 24)))
        dec += sum(2.0 * 2 * hwl * 128 * cin * 9 * 4 for hwl, cin in ((300, 256), (1200, 128), (4800, 128), (1200, 256), (4800, 128),
                                                                     (4800, 256), (19200, 256)))
        heads = sum(2.0 * 2 * 19200 * 128 * ch for ch in (7, 24, 18, 18))
        assert fl[0] == fl[1] == 2.0 * 2 * enc_macs + dec + heads and fl[2] == 0.0
    finally:
        hiplib.fpc_net_destroy(h)


def test_engine_refusals(hiplib):
    h = ctypes.c_void_p()
    assert hiplib.fpc_net_create(NAME.encode(), 7, 2, 481, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(NAME.encode(), 7, 2, 480, 650, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(NAME.encode(), 1, 2, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(NAME.encode(), 33, 2, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(NAME.encode(), 7, 0, 480, 640, ctypes.byref(h)) == -1
    for name in (b"efficientnet-b1", b"efficientnet_b0", b"efficientnet-b0 ", b"efficientnet"):
        assert hiplib.fpc_net_create(name, 7, 1, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(NAME.encode(), 32, 1, 32, 32, ctypes.byref(h)) == 0
    hiplib.fpc_net_destroy(h)
    assert hiplib.fpc_abi_version() == 11


def test_standalone_entries_refuse_bad_arguments_on_the_host(hiplib):
    """Everything the entries check before they launch: no device memory is touched (the 'pointers' are aligned integers)."""
    L = hiplib
    p = [4096 * (i + 1) for i in range(7)]
    pick = lambda base, kw, keys: [{**base, **kw}[k] for k in keys]
    dw = lambda a=None, **kw: L.fpc_mbconv_dw(*(a or p[:5]), *pick(dict(B=1, Hi=4, Wi=4, C=32, k=5, stride=2, act=2), kw,
                                                                     ("B", "Hi", "Wi", "C", "k", "stride", "act")), None)
    for bad in (dict(C=6), dict(C=0), dict(C=2), dict(k=4), dict(k=7), dict(k=1), dict(stride=3), dict(stride=0), dict(B=0), dict(act=3),
                dict(act=-1), dict(Hi=0), dict(Wi=0), dict(Hi=5), dict(Wi=7)):      # (odd extents at stride 2)
        assert dw(**bad) == -1, bad
    for i in range(5):
        a = list(p[:5]); a[i] = None
        assert dw(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert dw(a) == -1, ("misaligned", i)
    gate = lambda a=None, **kw: L.fpc_mbconv_gate(*(a or p[:7]), *pick(dict(B=2, H=4, W=4, C=96, Cs=4), kw, ("B", "H", "W", "C", "Cs")), None)
    for bad in (dict(C=6), dict(C=0), dict(C=2052), dict(Cs=0), dict(Cs=65), dict(B=0), dict(B=65536), dict(H=0), dict(W=0)):
        assert gate(**bad) == -1, bad
    for i in range(7):
        a = list(p[:7]); a[i] = None
        assert gate(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert gate(a) == -1, ("misaligned", i)
    # the slab count and the scratch size are functions of the shape alone
    assert [L.fpc_mbconv_gate_slabs(h, w, c) for h, w, c in ((15, 20, 1152), (1, 1, 32), (30, 40, 144), (120, 160, 96), (7, 3, 240),
                                                             (240, 320, 32))] == [10, 1, 6, 60, 1, 75]
    assert L.fpc_mbconv_gate_slabs(4, 4, 6) == 0 and L.fpc_mbconv_gate_slabs(0, 4, 8) == 0 and L.fpc_mbconv_gate_slabs(4, 4, 2052) == 0
    assert L.fpc_mbconv_gate_scratch_floats(3, 15, 20, 1152) == 3 * 10 * 1152 and L.fpc_mbconv_gate_scratch_floats(0, 15, 20, 1152) == 0
    # in, gate, w, scale, shift, res, out
    pw = lambda a=None, **kw: L.fpc_mbconv_pw(*(a or [p[0], None, p[2], p[3], p[4], None, p[6]]),
                                              *pick(dict(B=2, HW=3, Cin=1152, Cout=192, act=0), kw, ("B", "HW", "Cin", "Cout", "act")), None)
    for bad in (dict(Cin=12), dict(Cin=0), dict(Cin=2056), dict(Cout=12), dict(Cout=4), dict(Cout=2056), dict(B=0), dict(HW=0), dict(act=3),
                dict(act=-1), dict(B=2, HW=2 ** 30)):
        assert pw(**bad) == -1, bad
    assert pw(p[:7], act=2) == -1                                   # a residual together with an activation
    for i in (0, 2, 3, 4, 6):
        a = [p[0], None, p[2], p[3], p[4], None, p[6]]; a[i] = None
        assert pw(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert pw(a) == -1, ("misaligned", i)
    for i in (1, 5):                                                # gate and res may be NULL, not misaligned
        a = [p[0], None, p[2], p[3], p[4], None, p[6]]; a[i] = p[i] + 4
        assert pw(a) == -1, ("misaligned", i)
    # the form, as fpc_conv1x1_f32_form's for M = B HW; K = 1152 is taken here and refused there
    assert [L.fpc_mbconv_pw_form(b, hw, 1152, co) for b, hw, co in ((1, 300, 192), (3, 300, 192), (32, 300, 192), (32, 1200, 112),
                                                                   (3, 1380, 256), (2, 32761, 64), (2, 32761, 96), (2, 32761, 160))] == \
        [0, 0, 1, 2, 1, 2, 3, 5]      # (32 x 1200 rows, 112 channels: 1200 x 4 tiles, two per wave leave 2400 waves)
    assert L.fpc_mbconv_pw_form(1, 300, 1152, 192) == L.fpc_conv1x1_f32_form(300, 1024, 192) and L.fpc_conv1x1_f32_form(300, 1152, 192) == -1
    assert L.fpc_mbconv_pw_form(0, 300, 32, 16) == -1 and L.fpc_mbconv_pw_form(1, 300, 12, 16) == -1 and L.fpc_mbconv_pw_form(1, 300, 32, 4) == -1
    st = lambda a=None, **kw: L.fpc_mbconv_stem(*(a or p[:5]), *pick(dict(B=1, Hi=4, Wi=4, Cout=32), kw, ("B", "Hi", "Wi", "Cout")), None)
    for bad in (dict(Cout=64), dict(Cout=16), dict(B=0), dict(Hi=0), dict(Wi=0), dict(Hi=5), dict(Wi=3)):
        assert st(**bad) == -1, bad
    for i in range(5):
        a = list(p[:5]); a[i] = None
        assert st(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert st(a) == -1, ("misaligned", i)
