"""The transposed launch of k_conv_wino_h3 (fpc_conv2d's request -11, fpc_net_set_wino_orient): a site whose tile columns fill whole
8-column patches while its tile rows do not runs on the virtual image H' = W, W' = H with the weight image of the transposed taps,
and packs its frames along the stored image's y.  Only the staging plan's pixel offsets and the epilogue's output offsets know.

The smallest maps the rule transposes are 24 x 32 and 23 x 31: 12 tile rows x 16 tile columns, two frames per canvas row, three
patches per pair of frames with a seam in the middle one.  Outputs and records start from NaN: everything read later was written by
the launch.  The row and column halves of both transforms swap their order of additions, so a transposed launch equals the plain one
to rounding, not bit for bit — except on operands on which every intermediate is exact, and against the SAME kernel run on the
transposed tensors, where every difference is an indexing error."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_operands import _exact_case
from test_gpu_p2_fold import _check_seg6, _model
from test_gpu_wino_pack import _conv

pytestmark = pytest.mark.gpu

PLAIN, PACKED, ORIENT = -9, -10, -11


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


def _orient_geometry(H, W, B, Cin, fold=0, pack=1):
    from fastposecnn_amd import _native as nat
    out = (ctypes.c_int64 * 9)()
    nat.check(nat.lib().fpc_wino_orient_geometry(H, W, B, Cin, fold, pack, out), "geometry")
    return int(out[0]), dict(zip(("G", "tbx", "tby", "patches", "slots", "tiles", "gn_rows", "rx"), list(out)[1:]))


def _pack_geometry(H, W, B, Cin):
    from fastposecnn_amd import _native as nat
    out = (ctypes.c_int64 * 8)()
    nat.check(nat.lib().fpc_wino_pack_geometry(H, W, B, Cin, 0, out), "geometry")
    return dict(zip(("G", "tbx", "tby", "patches", "slots", "tiles", "gn_rows", "rx"), out))


SHAPES = [(B, Cin, H, W) for (H, W) in ((24, 32), (23, 31)) for B in (2, 3, 5) for Cin in (16, 48)]
EPILOGUES = ("bn_relu_res", "gn", "none")


def _operands(B, Cin, H, W, Cout, extra, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5
    scale = shift = res = None
    if "bn" in extra:
        scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    if "res" in extra:
        res = torch.randn((B, Cout, H, W), generator=g)
    return x, w, scale, shift, res


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d-%dx%dx%d" % s)
def test_transposed_launch_against_float64_and_against_itself_on_transposed_tensors(lib, dev, shape):
    """(i) request -11 against float64 at 2e-5 of scale, the records at the bar of test_gpu_wino_pack.py; (ii) the same launch must
    equal BIT FOR BIT request -10 (where that shape packs, else -9) on the H/W-transposed input with transposed taps, transposed
    back: the same kernel on the same virtual image."""
    B, Cin, H, W = shape
    Cout = 64
    tr, q = _orient_geometry(H, W, B, Cin)
    assert tr == 1 and q["G"] == 2 and q["patches"] == 2 * (3 * (B // 2) + 2 * (B % 2))
    t = lambda a: None if a is None else a.contiguous().to(dev)
    for extra in EPILOGUES:
        x, w, scale, shift, res = _operands(B, Cin, H, W, Cout, extra, 7 * SHAPES.index(shape) + EPILOGUES.index(extra))
        relu, gn = "relu" in extra, extra == "gn"
        xd, wd = x.permute(0, 2, 3, 1).contiguous().to(dev), w.contiguous().to(dev)
        resd = None if res is None else res.permute(0, 2, 3, 1).contiguous().to(dev)
        out, gp, P = _conv(dev, xd, wd, ORIENT, scale=t(scale), shift=t(shift), res=resd, relu=relu, gn=gn)
        assert P == q["gn_rows"]
        assert not torch.isnan(out).any(), "unwritten outputs"
        ref = F.conv2d(x.double(), w.double(), padding=1)
        if scale is not None:
            ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        if res is not None:
            ref = ref + res.double()
        if relu:
            ref = ref.relu()
        err = (out.permute(0, 3, 1, 2).cpu().double() - ref).abs().max().item()
        print(shape, extra, "float64 error", err, "scale", ref.abs().max().item())
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (extra, err)
        if gn:
            assert not torch.isnan(gp).any(), "a GroupNorm record the finalize kernel reads was not written"
            s = gp.cpu().double().sum(1)
            np.testing.assert_allclose(s[..., 0].numpy(), ref.sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3)
            np.testing.assert_allclose(s[..., 1].numpy(), (ref * ref).sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3)
        # (ii) the same kernel, fed the transposed tensors
        sibling = PACKED if _pack_geometry(W, H, B, Cin)["G"] > 1 else PLAIN
        assert sibling == PACKED
        xt = xd.permute(0, 2, 1, 3).contiguous()                       # [B, W, H, Cin]
        wt = wd.permute(0, 1, 3, 2).contiguous()
        rest = None if resd is None else resd.permute(0, 2, 1, 3).contiguous()
        out_t, gp_t, P_t = _conv(dev, xt, wt, sibling, scale=t(scale), shift=t(shift), res=rest, relu=relu, gn=gn)
        assert torch.equal(out, out_t.permute(0, 2, 1, 3)), "request -11 differs from the same launch on the transposed tensors: " + extra
        if gn:
            assert P_t == P and torch.equal(gp, gp_t)


@pytest.mark.parametrize("shape", [(2, 16, 24, 32, 64, 3, 1, 1), (3, 48, 23, 31, 64, 3, 1, 1), (5, 16, 23, 31, 128, 3, 1, 1)],
                         ids=lambda s: "b%d-%dx%dx%d-%d" % s[:5])
def test_transposed_launch_is_exact_on_single_piece_operands(lib, dev, shape):
    """(iii) operands on the first exact grid of tests/test_gpu_conv_operands.py (every product and every sum exact, whatever the
    order of additions): request -11 equals float64, and therefore the plain -9 launch, bit for bit."""
    from test_gpu_net import _conv2d
    assert _orient_geometry(shape[2], shape[3], shape[0], shape[1])[0] == 1
    x, w, kw, ref = _exact_case(shape, "wino", 0)
    out = _conv2d(dev, x, w, 1, 1, nsplit=ORIENT, **kw)[0]
    plain = _conv2d(dev, x, w, 1, 1, nsplit=PLAIN, **kw)[0]
    assert torch.equal(out, ref.float()), "request -11 is not exact on the grid"
    assert torch.equal(out, plain)


def test_request_on_a_shape_the_rule_leaves_alone_is_the_plain_launch(lib, dev):
    g = torch.Generator().manual_seed(5)
    for B, H, W in ((4, 15, 20), (3, 12, 32), (2, 32, 24)):
        assert _orient_geometry(H, W, B, 32)[0] == 0
        xd = torch.randn((B, H, W, 32), generator=g).to(dev)
        wd = (torch.randn((64, 32, 3, 3), generator=g) / 17.0).to(dev)
        a, ga, Pa = _conv(dev, xd, wd, PLAIN, gn=True)
        b, gb, Pb = _conv(dev, xd, wd, ORIENT, gn=True)
        assert Pa == Pb and torch.equal(a, b) and torch.equal(ga, gb)


# ---- the network: ResNet18 at 96 x 128 is the smallest pyramid on which the rule fires (c2 / p2 = 24 x 32; 12 x 16 has fewer than
# 8 tile rows): layer1's four sites and the folded s2.0 (p3 = 12 x 16) run transposed

def _small_engine(lib, dev, B, graph=False):
    from fastposecnn_amd.engine import NetEngine
    m, hp = _model(lib, "resnet18")
    md = copy.deepcopy(m).to(dev)
    eng = NetEngine(md, B, 96, 128, dev, autotune=False, graph=graph, split_precision=3)
    eng.force_winograd(9)
    eng.force_fold(1)
    return m, hp, md, eng


@pytest.mark.parametrize("B", [2, 3])
def test_fold_transposed_against_float64(lib, dev, B):
    """(iv) s2.0 with p2 folded in, transposed and packed (p2 24 x 32, p3 12 x 16; B = 3: the last canvas row holds one frame, its
    second patch is cut at the frame's end): the pre-GroupNorm output within 2e-5 of float64 of the engine's own c2 and p3, with
    orientation on and off."""
    from fastposecnn_amd import synth
    m, hp, md, eng = _small_engine(lib, dev, B)
    x = torch.stack([synth.make_image(i, 96, 128) for i in range(B)]).to(dev)
    for on in (1, 0, 1):
        eng.set_wino_orient(on)
        with torch.no_grad():
            eng.forward(x)
        torch.cuda.synchronize()
        assert any(p[2] == 5000 for p in eng.conv_plans())
        _check_seg6(md, eng, list(range(B)))


def test_network_orientation_on_and_off(lib, dev):
    """(v) ResNet18, 96 x 128, B = 3, every 3x3 / stride-1 site on form 9 and the fold kept: logits within 1e-4 of the float64 module
    path; orientation on and off within 2e-5 of scale of each other; plans and workspace identical; the form-9 workgroups drop by
    the geometry's figure; set_wino_pack makes the same difference either way; switching back restores the first run bit for bit."""
    from fastposecnn_amd import synth
    B = 3
    m, hp, md, eng = _small_engine(lib, dev, B)
    x = torch.stack([synth.make_image(i, 96, 128) for i in range(B)])
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp); ref_m.HPARAM.USE_NATIVE_ENGINE = False
    with torch.no_grad():
        ref = ref_m.pure_model_forward(x.double())
    xd = x.to(dev)
    plans, wsb = eng.conv_plans(), eng._lib.fpc_net_workspace_bytes(eng._h)
    runs, blocks = [], {}
    for orient, pack in ((1, 1), (0, 1), (1, 0), (0, 0), (1, 1)):
        eng.set_wino_orient(orient)
        eng.set_wino_pack(pack)
        with torch.no_grad():
            logits, _ = eng.forward(xd)
        torch.cuda.synchronize()
        assert eng.conv_plans() == plans and eng._lib.fpc_net_workspace_bytes(eng._h) == wsb
        runs.append({k: v.clone() for k, v in logits.items()})
        blocks[(orient, pack)] = eng.wino_blocks()
    on, off = runs[0], runs[1]
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        scale = max(1.0, ref[k].abs().max().item())
        err = (on[k].cpu().double() - ref[k]).abs().max().item()
        diff = (on[k] - off[k]).abs().max().item()
        print(k, "float64 error", err, "scale", scale, "on - off", diff)
        assert err <= 1e-4 * scale, (k, err, scale)
        assert diff <= 2e-5 * scale, (k, diff, scale)
        assert torch.equal(runs[0][k], runs[4][k]), k
    # layer1: 4 sites x 1 channel block; the folded s2.0: 2 channel blocks x 4 decoders
    tr, q = _orient_geometry(24, 32, B, 64)
    saved = (_pack_geometry(24, 32, B, 64)["patches"] - q["patches"]) * (4 * 1 + 2 * 4)
    assert tr == 1 and saved == 2 * 12
    print("form-9 workgroups", blocks)
    assert blocks[(0, 1)] - blocks[(1, 1)] == saved and blocks[(0, 0)] - blocks[(1, 0)] == saved
    assert blocks[(1, 0)] - blocks[(1, 1)] == blocks[(0, 0)] - blocks[(0, 1)]


def test_network_transposed_graph_replay_bit_equal(lib, dev):
    """The recorded graph replays the plain launches' logits bit for bit with the transposed sites in it."""
    from fastposecnn_amd import synth
    xs = [torch.stack([synth.make_image(i + j, 96, 128) for j in range(3)]).to(dev) for i in range(2)]
    side = torch.cuda.Stream(device=dev)
    runs = []
    for graph in (False, True):
        with torch.no_grad(), torch.cuda.stream(side):
            m, hp, md, eng = _small_engine(lib, dev, 3, graph=graph)
            outs = []
            for x in xs + xs:
                logits, _ = eng.forward(x)
                outs.append({k: v.clone() for k, v in logits.items()})
        side.synchronize()
        assert eng.graph_recorded() == graph
        runs.append(outs)
        del eng
    for a, b in zip(*runs):
        for k in a:
            assert torch.equal(a[k], b[k]), k
