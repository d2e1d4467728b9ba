"""CPU checks of the VGG encoders (vgg11 / 13 / 16 / 19 and each with _bn): the module restatement against the published definition
of torchvision's vgg.make_layers as smp's VGGEncoder wraps it (parameter counts and state-dict key lists computed here from the
configuration table, feature levels, the forward in float64 against a plain F.conv2d / F.max_pool2d restatement), the names, the
preprocessing parameters, the engine's host-side plan (fpc_net_create("vgg16" ...): parameter table, convolution count, refusals,
the size bound), the host-side refusals of the two stand-alone kernel entries, and the condition the GPU engine test puts on its own
inputs.  No compute calls into the HIP library."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _vgg_model as V

NAMES = V.NAMES
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def by_table(name):
    """(parameters, state-dict keys in order, [(features index of the conv, Cin, Cout)] per block) from the configuration table:
    a convolution takes two indices of the Sequential (three with BatchNorm), a pool one."""
    bn = name.endswith("_bn")
    total, keys, blocks, idx, cin = 0, [], [], 0, 3
    for n, c in zip(V.CONFIGS[name[:5]], V.CHANNELS):
        blocks.append([])
        for _ in range(n):
            total += c * cin * 9 + c
            keys += [f"features.{idx}.weight", f"features.{idx}.bias"]
            blocks[-1].append((idx, cin, c))
            if bn:
                total += 2 * c
                keys += [f"features.{idx + 1}.{k}" for k in BN_KEYS]
            idx += 3 if bn else 2
            cin = c
        idx += 1
    return total, keys, blocks


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


def test_the_table_gives_the_published_counts():
    assert by_table("vgg16")[0] == 14_714_688 and len(by_table("vgg16")[1]) == 26
    assert by_table("vgg16_bn")[0] == 14_723_136 and len(by_table("vgg16_bn")[1]) == 91
    assert [sum(V.CONFIGS[n]) for n in ("vgg11", "vgg13", "vgg16", "vgg19")] == [8, 10, 13, 16]


@pytest.mark.parametrize("name", NAMES)
def test_parameters_and_state_dict_keys(encs, name):
    total, keys, blocks = by_table(name)
    enc = encs[name]
    assert sum(p.numel() for p in enc.parameters()) == total
    sd = enc.state_dict()
    assert list(sd) == keys
    idx = [int(k.split(".")[1]) for k in keys]
    assert idx == sorted(idx)                                           # key order is features.N order
    for i, cin, c in (s for b in blocks for s in b):
        assert tuple(sd[f"features.{i}.weight"].shape) == (c, cin, 3, 3) and tuple(sd[f"features.{i}.bias"].shape) == (c,)
    assert not any(k.startswith(("classifier", "avgpool")) for k in keys)


@pytest.mark.parametrize("name", NAMES)
def test_module_properties_and_forward_against_the_formula(encs, name):
    from fastposecnn_amd.lib import backbone as bb
    _, _, blocks = by_table(name)
    bn = name.endswith("_bn")
    enc = encs[name]
    assert isinstance(enc, bb.VGGEncoder) and enc.name == name and enc.out_channels == (64, 128, 256, 512, 512, 512)
    assert isinstance(enc.features, torch.nn.Sequential) and not hasattr(enc, "classifier") and not hasattr(enc, "avgpool")
    mods = list(enc.features)
    assert len(mods) == sum(len(b) for b in blocks) * (3 if bn else 2) + 5
    for b in blocks:
        for i, cin, c in b:
            conv = mods[i]
            assert isinstance(conv, bb.Conv2d) and conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.stride == (1, 1) and conv.bias is not None
            if bn:
                assert isinstance(mods[i + 1], bb.BatchNorm2d) and mods[i + 1].eps == 1e-5 and mods[i + 1].momentum == 0.1
            assert isinstance(mods[i + (2 if bn else 1)], torch.nn.ReLU)
        pool = mods[b[-1][0] + (3 if bn else 2)]
        assert isinstance(pool, torch.nn.MaxPool2d) and pool.kernel_size == 2 and pool.stride == 2 and pool.padding == 0
    assert isinstance(mods[-1], torch.nn.MaxPool2d)
    # the forward in float64 against a plain restatement: a level per block in front of its pool, then the last pool alone
    e64 = bb.VGGEncoder(name).double().eval()
    g = torch.Generator().manual_seed(5)
    for m in e64.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.bias.data.copy_(torch.randn(m.out_channels, generator=g, dtype=torch.float64) * 0.1)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.3)
    x = torch.randn((1, 3, 64, 96), generator=g, dtype=torch.float64)
    with torch.no_grad():
        feats = e64(x.clone())
        sd = e64.state_dict()
        want, y = [], x
        for b in blocks:
            for i, _, _ in b:
                y = F.conv2d(y, sd[f"features.{i}.weight"], sd[f"features.{i}.bias"], 1, 1)
                if bn:
                    v = lambda k: sd[f"features.{i + 1}.{k}"].double().view(1, -1, 1, 1)
                    y = (y - v("running_mean")) / torch.sqrt(v("running_var") + 1e-5) * v("weight") + v("bias")
                y = y.clamp_min(0)
            want.append(y)
            y = F.max_pool2d(y, 2, 2)
        want.append(y)
    assert len(feats) == 6
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 64, 96), (128, 32, 48), (256, 16, 24), (512, 8, 12), (512, 4, 6), (512, 2, 3)]
    assert feats[0].shape != x.shape and feats[0].shape[1] == 64          # the first level is block 1's output, not the input image
    for f, w in zip(feats, want):
        assert torch.allclose(f, w, rtol=0, atol=1e-12 * max(1.0, w.abs().max().item()))
    assert torch.equal(feats[5], F.max_pool2d(feats[4], 2, 2))              # the last level: the last pool alone


def test_names():
    from fastposecnn_amd.lib import backbone as bb
    from fastposecnn_amd.tools import dataset
    for name in NAMES:
        assert bb.encoder_family(name) == "vgg" and name in bb._available()
        assert dataset.get_preprocessing_params(name) == dataset.get_preprocessing_params("resnet18")
    assert bb.encoder_family("resnet18") == "resnet" and bb.encoder_family("densenet121") == "densenet"
    for other in ("vgg16bn", "vgg", "vgg21", "vgg16_bn "):
        with pytest.raises(KeyError):
            bb.encoder_family(other)
        with pytest.raises(KeyError, match="vgg16_bn"):      # the message lists what there is
            bb.get_encoder(other)
        with pytest.raises(ValueError):
            dataset.get_preprocessing_params(other)
        assert other not in bb._available()


@pytest.mark.parametrize("name", NAMES)
def test_engine_param_table_matches_state_dict(hiplib, name):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = name
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    total, keys, blocks = by_table(name)
    nconv = sum(len(b) for b in blocks)
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
        order = ["encoder." + k for k in keys if not k.endswith("num_batches_tracked")]
        assert [nm for nm in names if nm.startswith("encoder.")] == order
        assert order == [k for k in m.state_dict() if k.startswith("encoder.") and not k.endswith("num_batches_tracked")]
        assert sum(hiplib.fpc_net_param_numel(h, i) for i, nm in enumerate(names)
                   if nm.startswith("encoder.") and not nm.endswith(("running_mean", "running_var"))) == total
        assert names.index("mask_decoder.p5.weight") == len(order)         # then the decoders and heads, as on every plan
        assert hiplib.fpc_net_workspace_bytes(h) > 0
        assert hiplib.fpc_net_forward(h, *([None] * 11), None) == -1          # before load_params: refused, not a crash
        assert hiplib.fpc_net_force_fold(h, 1) == -1 and hiplib.fpc_net_force_fold(h, 0) == 0
        assert hiplib.fpc_net_force_stem_pool(h, 1) == -1 and hiplib.fpc_net_force_stem_pool(h, 0) == -1      # there is no 7x7 stem
        # the convolution sites: the encoder's convolutions but features.0, then the decoders' 4 x (4 laterals + 7 segmentation convolutions)
        assert hiplib.fpc_net_conv_count(h) == nconv - 1 + 44
        if name == "vgg16":
            assert hiplib.fpc_net_conv_count(h) == 56
        out = (ctypes.c_int * 5)()
        plans = []
        for i in range(hiplib.fpc_net_conv_count(h)):
            assert hiplib.fpc_net_conv_plan(h, i, out) == 0
            plans.append(tuple(out))
        sites = [(cin, c) for b in blocks for _, cin, c in b][1:]
        assert [(p[4] // 9, p[3]) for p in plans[:nconv - 1]] == sites
        assert [p[4] for p in plans[nconv - 1:nconv + 3]] == [512, 512, 512, 256] and all(p[3] == 256 for p in plans[nconv - 1:nconv + 3])
        # FLOP of a frame pair: the encoder by arithmetic beside the decoder sites and the heads
        fl = (ctypes.c_double * 3)()
        assert hiplib.fpc_net_flops(h, fl) == 0
        macs, hw = 0, 480 * 640
        for b in blocks:
            macs += sum(hw * cin * c * 9 for _, cin, c in b)
            hw //= 4
        dec = sum(2.0 * 2 * hwl * 256 * cin * 4 for hwl, cin in ((300, 512), (1200, 512), (4800, 512), (19200, 256)))
        dec += sum(2.0 * 2 * hwl * 128 * cin * 9 * 4 for hwl, cin in ((300, 256), (1200, 128), (4800, 128), (1200, 256), (4800, 128),
                                                                     (4800, 256), (19200, 256)))
        heads = sum(2.0 * 2 * 19200 * 128 * ch for ch in (7, 24, 18, 18))
        assert fl[0] == 2.0 * 2 * macs + dec + heads
    finally:
        hiplib.fpc_net_destroy(h)


def test_engine_refusals(hiplib):
    h = ctypes.c_void_p()
    for name in NAMES:
        assert hiplib.fpc_net_create(name.encode(), 7, 2, 481, 640, ctypes.byref(h)) == -1
        assert hiplib.fpc_net_create(name.encode(), 7, 2, 480, 650, ctypes.byref(h)) == -1
        assert hiplib.fpc_net_create(name.encode(), 1, 2, 480, 640, ctypes.byref(h)) == -1
        assert hiplib.fpc_net_create(name.encode(), 33, 2, 480, 640, ctypes.byref(h)) == -1
        assert hiplib.fpc_net_create(name.encode(), 7, 0, 480, 640, ctypes.byref(h)) == -1
    for name in (b"vgg16bn", b"vgg", b"vgg21", b"vgg16_bn "):
        assert hiplib.fpc_net_create(name, 7, 1, 480, 640, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create(b"vgg19_bn", 32, 1, 32, 32, ctypes.byref(h)) == 0
    hiplib.fpc_net_destroy(h)
    assert hiplib.fpc_abi_version() == 11


def test_size_bound(hiplib):
    """a VGG plan is built while 16 B H W < 2^32 - 2^20 - 8 (features.0's walk over the batch) and
    (H + 2) W 256 < 2^31 (the implicit GEMM's lane offsets in one full-resolution 64-channel frame), refused beyond.  The headline
    batch, 32 x 480 x 640, is built; 873 frames of 640 x 480 are the most."""
    limit = 2 ** 32 - 2 ** 20 - 8
    h = ctypes.c_void_p()

    def built(B, H, W):
        rc = hiplib.fpc_net_create(b"vgg16_bn", 7, B, H, W, ctypes.byref(h))
        if rc == 0:
            hiplib.fpc_net_destroy(h)
        assert rc in (0, -1)
        return rc == 0

    assert built(32, 480, 640)
    assert 16 * 873 * 480 * 640 < limit <= 16 * 874 * 480 * 640
    assert built(873, 480, 640) and not built(874, 480, 640)
    # per frame: H + 2 < 2^31 / (256 W); at W = 32 the last multiple of 32 inside is 262 112
    assert (262112 + 2) * 32 * 256 < 2 ** 31 <= (262144 + 2) * 32 * 256
    assert built(1, 262112, 32) and not built(1, 262144, 32)


def test_standalone_entries_refuse_bad_arguments_on_the_host(hiplib):
    """Everything the two entries check before they launch: no device memory is touched (the 'pointers' are aligned integers)."""
    L = hiplib
    p = [4096 * (i + 1) for i in range(5)]
    pick = lambda base, kw, keys: [{**base, **kw}[k] for k in keys]
    # in4, w, scale, shift, out
    cv = lambda a=None, **kw: L.fpc_conv3x3_c3(*(a or p), *pick(dict(B=2, H=5, W=7, Cout=64, act=1), kw, ("B", "H", "W", "Cout", "act")), None)
    for bad in (dict(Cout=32), dict(Cout=128), dict(Cout=0), dict(B=0), dict(H=0), dict(W=0), dict(act=2), dict(act=-1),
                dict(B=2 ** 10, H=2 ** 9, W=2 ** 9), dict(B=874, H=480, W=640)):
        assert cv(**bad) == -1, bad
    for i in (0, 1, 3, 4):                          # (scale may be NULL: the bias alone)
        a = list(p); a[i] = None
        assert cv(a) == -1, ("null", i)
    for i in range(5):
        a = list(p); a[i] = p[i] + 4
        assert cv(a) == -1, ("misaligned", i)
    # x, y
    mp = lambda a=None, **kw: L.fpc_maxpool2x2_fwd(*(a or p[:2]), *pick(dict(B=2, H=6, W=10, C=64), kw, ("B", "H", "W", "C")), None)
    for bad in (dict(H=5), dict(W=9), dict(H=0), dict(W=0), dict(B=0), dict(C=6), dict(C=2), dict(C=0), dict(C=-4),
                dict(B=2 ** 10, H=2 ** 11, W=2 ** 11, C=64)):
        assert mp(**bad) == -1, bad
    for i in range(2):
        a = list(p[:2]); a[i] = None
        assert mp(a) == -1, ("null", i)
        a[i] = p[i] + 4
        assert mp(a) == -1, ("misaligned", i)


@pytest.mark.parametrize("encoder,B,H,W", V.ENGINE_CASES)
def test_the_engine_tests_draw_is_well_conditioned(encoder, B, H, W):
    """What tests/test_gpu_vgg.py::test_engine_vs_float64_cpu asks of its own inputs: with its parameter draw (seed V.SEED), torch's
    f32 CPU forward of the module stays within a quarter of the network bar 1e-4 max(1, |ref|max) of float64 on all six feature levels
    and every logit, so the bar measures the engine and not the conditioning of the draw; and the activations the 3x3 sites read stay
    O(1): far inside the fp16-piece forms' stated range (2^-2 .. 2^16 for the bulk)."""
    import fastposecnn_amd.lib as L
    errs = V.f32_errors(L, encoder, V.images(B, H, W))
    for err, scale in errs:
        assert err <= 0.25 * 1e-4 * max(1.0, scale), (err, scale)
    assert all(2.0 ** -2 < scale < 2.0 ** 8 for _, scale in errs[:6]), [s for _, s in errs[:6]]
