"""The packed geometry of k_conv_wino_h3 (fpc_conv2d's request -10, fpc_net_set_wino_pack): the frames of a small map lie side by
side on a canvas row and the 8 x 8 tile patches are cut out of the canvas, so fewer workgroups run their K loop on empty tile
columns.  The per-tile arithmetic is form -9's own (the same products in the same order), so the outputs must equal the plain -9
launch BIT FOR BIT; the GroupNorm records are summed per (frame, patch) in another grouping and agree to rounding.  Outputs and
records start from NaN: everything read later was written by the launch."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PLAIN, PACKED = -9, -10


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


def _cdiv(a, b):
    return -(-a // b)


def _geometry(H, W, B, Cin):
    from fastposecnn_amd import _native as nat
    out = (ctypes.c_int64 * 8)()
    nat.check(nat.lib().fpc_wino_pack_geometry(H, W, B, Cin, 0, out), "geometry")
    return dict(zip(("G", "tbx", "tby", "patches", "slots", "tiles", "gn_rows", "rx"), out))


def _conv(dev, xd, wd, nsplit, scale=None, shift=None, res=None, relu=False, gn=False):
    """3x3 / stride 1 / pad 1 through fpc_conv2d on device tensors (x, res NHWC).  Returns (out NHWC, records or None, P32)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, H, W, Cin = xd.shape
    Cout = wd.shape[0]
    plan = (ctypes.c_int * 4)()
    nat.check(L.fpc_conv2d_plan(B, H, W, Cin, Cout, 3, 3, 0, 0, nsplit, plan), "plan")
    assert plan[2] == nsplit
    out = torch.full((B, H, W, Cout), float("nan"), device=dev)
    gpart = torch.full((B, plan[3], Cout, 2), float("nan"), device=dev) if gn else None
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, H, W, Cin, Cout, 3, 3), dtype=torch.uint8, device=dev)
    sb, sh, sw, sc = xd.stride()
    nat.check(L.fpc_conv2d(xd.data_ptr(), sb, sh, sw, sc, wd.data_ptr(), nat.ptr(scale), nat.ptr(shift), nat.ptr(res), None,
                           out.data_ptr(), nat.ptr(gpart), B, H, W, Cin, Cout, 3, 3, 1, 1, int(relu), 0, 0, nsplit, ws.data_ptr(),
                           ws.numel(), nat.stream()), "conv2d")
    torch.cuda.synchronize()
    return out, gpart, plan[3]


# B, Cin, H, W, Cout, epilogue, frames held to float64 (None: all)
CASES = [
    (32, 512, 15, 20, 512, "bn_relu_res", (0, 3, 4, 31)),   # layer4: four frames per canvas row, 5 patches instead of 8
    (32, 256, 30, 40, 256, "bn_relu_res", (0, 1, 30, 31)),  # layer3: two frames per canvas row, 5 patches instead of 6
    (5, 256, 30, 40, 128, "gn", None),                      # ragged: the last canvas row holds one frame
    (7, 256, 15, 20, 128, "gn", None),                      # ragged: the last canvas row holds three frames of four
    (4, 32, 9, 17, 64, "bn", None),                         # odd width: 9 tile columns, the last one half empty, seams at every offset
    (6, 48, 12, 22, 64, "gn", None),                        # 11 tile columns, three pairs of K-steps (the staging ring wraps)
    (3, 16, 15, 20, 64, "bias_relu", None),                 # a single pair of K-steps; three frames, G = 3
    (32, 256, 15, 20, 128, "gn", (0, 5, 31)),               # s5.0
    (32, 128, 30, 40, 128, "gn", (0, 17, 31)),              # s5.1
    (32, 256, 30, 40, 128, "gn", (0, 17, 31)),              # s4.0
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"b{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}-{c[5]}")
def test_packed_launch_equals_plain_and_meets_float64(lib, dev, case):
    B, Cin, H, W, Cout, extra, frames = case
    g = torch.Generator().manual_seed(CASES.index(case) + 100)
    x = torch.randn((B, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5
    scale = shift = res = None
    if "bn" in extra:
        scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    if "bias" in extra:
        shift = torch.randn(Cout, generator=g)
    if "res" in extra:
        res = torch.randn((B, Cout, H, W), generator=g)
    relu, gn = "relu" in extra, extra == "gn"
    q = _geometry(H, W, B, Cin)
    assert q["G"] > 1, "the case does not pack"
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = w.contiguous().to(dev)
    t = lambda a: None if a is None else a.contiguous().to(dev)
    kw = dict(scale=t(scale), shift=t(shift), res=None if res is None else res.permute(0, 2, 3, 1).contiguous().to(dev), relu=relu, gn=gn)
    plain, gp_plain, P_plain = _conv(dev, xd, wd, PLAIN, **kw)
    packed, gp_packed, P_packed = _conv(dev, xd, wd, PACKED, **kw)
    assert P_plain == _cdiv(_cdiv(W, 2), 8) * _cdiv(_cdiv(H, 2), 8) and P_packed == q["gn_rows"]
    assert not torch.isnan(packed).any(), "unwritten outputs"
    assert torch.equal(packed, plain), "the packed launch is not bit-identical to the plain one"
    sel = list(range(B)) if frames is None else list(frames)
    ref = F.conv2d(x[sel].double(), w.double(), padding=1)
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        ref = ref + shift.double().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res[sel].double()
    if relu:
        ref = ref.relu()
    got = packed[sel].permute(0, 3, 1, 2).cpu().double()
    err = (got - ref).abs().max().item()
    print("float64 error", err, "scale", ref.abs().max().item())
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err
    if gn:
        assert not torch.isnan(gp_packed).any(), "a GroupNorm record the finalize kernel reads was not written"
        s = gp_packed[sel].cpu().double().sum(1)                    # [frames, Cout, 2] over the frame's records, as k_gn_finalize sums
        np.testing.assert_allclose(s[..., 0].numpy(), ref.sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(s[..., 1].numpy(), (ref * ref).sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3)
        sp = gp_plain[sel].cpu().double().sum(1)
        np.testing.assert_allclose(s.numpy(), sp.numpy(), rtol=1e-5, atol=1e-4)      # another grouping of the same f32 values


def test_packed_request_on_a_shape_that_cannot_pack_is_the_plain_launch(lib, dev):
    """7 tile columns (a patch could straddle three frames) and a single frame: -10 runs the plain geometry."""
    for B, H, W in ((4, 12, 14), (1, 15, 20)):
        g = torch.Generator().manual_seed(B)
        xd = torch.randn((B, H, W, 32), generator=g).to(dev)
        wd = (torch.randn((64, 32, 3, 3), generator=g) / 17.0).to(dev)
        assert _geometry(H, W, B, 32)["G"] == 1
        a, ga, Pa = _conv(dev, xd, wd, PLAIN, gn=True)
        b, gb, Pb = _conv(dev, xd, wd, PACKED, gn=True)
        assert Pa == Pb and torch.equal(a, b) and torch.equal(ga, gb)


def test_packed_repeat_bit_identical(lib, dev):
    g = torch.Generator().manual_seed(9)
    xd = torch.randn((8, 30, 40, 128), generator=g).to(dev)
    wd = (torch.randn((128, 128, 3, 3), generator=g) / 34.0).to(dev)
    a, ga, _ = _conv(dev, xd, wd, PACKED, gn=True)
    b, gb, _ = _conv(dev, xd, wd, PACKED, gn=True)
    assert torch.equal(a, b) and torch.equal(ga, gb)


# ---- the network

def _model(lib, seed=0):
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet34"
    hp.PERFORM_AGGREGATION = False
    torch.manual_seed(seed)
    m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
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
    return m.eval(), hp


# form-9 workgroups the packed geometry saves at ResNet34 / batch 32 / 640 x 480 with every 3x3 / stride-1 site on form 9:
# layer4 5 x (512 - 320) + s5.0 (512 - 320) + layer3 11 x (768 - 640) + s4.0 and s5.1 2 x (1 536 - 1 280)
SAVED_BLOCKS = 5 * 192 + 192 + 11 * 128 + 2 * 256


def test_network_batch32_packed_against_float64_and_against_plain(lib, dev):
    """ResNet34, B = 32, 640 x 480 (bench.py's headline) as the model builds it (autotuned, packing on by default): logits of
    frames 0 and 31 within 1e-4 of the float64 module path; the same engine with packing off gives every encoder tensor bit for
    bit and logits within 1e-5 of scale (the GroupNorm sums of three sites are the same f32 values added in another grouping: a
    relative change of a few 2^-24 per sum, far below the 1e-4 bar the logits are held to); the switch changes the grids.  ~90 s of float64 convolutions on the host."""
    from fastposecnn_amd import synth
    m, hp = _model(lib)
    x2 = torch.stack([synth.make_image(0), synth.make_image(31)])
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp); ref_m.HPARAM.USE_NATIVE_ENGINE = False
    with torch.no_grad():
        ref = ref_m.pure_model_forward(x2.double())
    del ref_m
    m = m.to(dev)
    x32 = torch.stack([synth.make_image(i) for i in range(32)]).to(dev)
    with torch.no_grad():
        m(x32)
    eng = m._engines[(32, 480, 640, x32.device)]
    plans = eng.conv_plans()
    n9 = sum(1 for p in plans if p[2] == -9)
    print("form-9 sites:", n9)
    assert n9 >= 20, "the headline plans are not on form 9"
    runs = {}
    for on in (1, 0, 1):
        eng.set_wino_pack(on)
        with torch.no_grad():
            logits, _ = eng.forward(x32)
        torch.cuda.synchronize()
        assert eng.conv_plans() == plans                     # packing is a property of the launch, not of the plan
        runs[on] = ({k: v.clone() for k, v in logits.items()}, {k: eng.tensor(k).clone() for k in ("c2", "c3", "c4", "c5")},
                    eng.wino_blocks())
    on, off = runs[1], runs[0]
    print("form-9 workgroups: packed", on[2], "plain", off[2])
    assert 0 < on[2] < off[2]
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = on[0][k][[0, 31]].cpu().double()
        scale = max(1.0, ref[k].abs().max().item())
        err = (got - ref[k]).abs().max().item()
        print(k, "float64 error", err, "scale", scale, "packed - plain", (on[0][k] - off[0][k]).abs().max().item())
        assert err <= 1e-4 * scale, (k, err, scale)
        assert (on[0][k] - off[0][k]).abs().max().item() <= 1e-5 * scale, k
    for k in ("c2", "c3", "c4", "c5"):
        assert torch.equal(on[1][k], off[1][k]), k
    del m._engines[(32, 480, 640, x32.device)]
    torch.cuda.empty_cache()


def test_switch_restores_the_plain_grids(lib, dev):
    """Every 3x3 / stride-1 site on form 9, the fold kept: packing saves exactly the workgroups the geometry promises and
    set_wino_pack(0) gives them back; a batch-1 engine has nothing to pack."""
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m, _ = _model(lib)
    m = m.to(dev)
    x = torch.stack([synth.make_image(i) for i in range(32)]).to(dev)
    eng = NetEngine(m, 32, 480, 640, dev, autotune=False, split_precision=3)
    eng.force_winograd(9)
    eng.force_fold(1)
    blocks = {}
    for on in (1, 0):
        eng.set_wino_pack(on)
        with torch.no_grad():
            eng.forward(x)
        torch.cuda.synchronize()
        blocks[on] = eng.wino_blocks()
    assert blocks[0] - blocks[1] == SAVED_BLOCKS, blocks
    del eng
    e1 = NetEngine(m, 1, 480, 640, dev, autotune=False, split_precision=3)
    e1.force_winograd(9)
    for on in (1, 0):
        e1.set_wino_pack(on)
        with torch.no_grad():
            e1.forward(x[:1])
        torch.cuda.synchronize()
        blocks[on] = e1.wino_blocks()
    assert blocks[0] == blocks[1] > 0


def test_network_packed_graph_replay_bit_equal(lib, dev):
    """ResNet34 at batch 32 with every 3x3 / stride-1 site on form 9 and packing on: the recorded graph replays the plain launches'
    logits bit for bit, and repeats are bit-identical."""
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m, _ = _model(lib)
    m = m.to(dev)
    xs = [torch.stack([synth.make_image(i + j) for j in range(32)]).to(dev) for i in range(2)]
    side = torch.cuda.Stream(device=dev)
    runs = []
    for graph in (False, True):
        with torch.no_grad(), torch.cuda.stream(side):
            eng = NetEngine(m, 32, 480, 640, dev, autotune=False, graph=graph, split_precision=3)
            eng.force_winograd(9)
            eng.force_fold(1)
            eng.set_wino_pack(1)
            outs = []
            for x in xs + xs:
                logits, _ = eng.forward(x)
                outs.append({k: v.clone() for k, v in logits.items()})
        side.synchronize()
        assert eng._lib.fpc_net_graph_recorded(eng._h) == (1 if graph else 0)
        runs.append(outs)
        del eng
    for a, b in zip(*runs):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[0][2][k]), k
