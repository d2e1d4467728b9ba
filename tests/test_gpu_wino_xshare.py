"""The x-shared tile map of the packed k_conv_wino_h3 launches (csrc/wino_tile.hpp, XS: a lane's two tiles are neighbours in x and
share half their input columns) against the row-split map requested explicitly (fpc_conv2d's -12 / -13 beside -10 / -11,
fpc_net_set_wino_xshare).  The map changes which lane holds which tile and where a tile's data lies in LDS; every product, every sum
and every order of summation is the same, so outputs and GroupNorm records must be EQUAL, bit for bit.  Outputs and records start
from NaN: everything compared was written by the launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PACKED, ORIENT, PACKED_ROWSPLIT, ORIENT_ROWSPLIT = -10, -11, -12, -13
CINS, COUTS = (16, 32, 48), (64, 128)
EPILOGUES = ("none", "bn_res_relu", "gn")
# (H, W, B): one patch without a seam; 24 x 32 and 23 x 31 run transposed under -11 (12 tile columns of the virtual image: two
# frames per canvas row, a seam after 4, a ragged last canvas row at B = 3 and 5, border patches on all four sides); 40 x 24
# packs under -10 (12 tile columns).  30 x 20 at B = 5: 10 tile columns, four frames per canvas row, seams after 2, 4 and 6.
SHAPES = [(16, 16, 1)] + [(h, w, b) for (h, w) in ((24, 32), (23, 31), (40, 24)) for b in (2, 3, 5)] + [(30, 20, 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat(dev):
    from fastposecnn_amd import _native
    _native.lib()
    return _native


def _conv(nat, dev, xd, wd, code, scale=None, shift=None, res=None, relu=False, gn=False):
    L = nat.lib()
    B, H, W, Cin = xd.shape
    Cout = wd.shape[0]
    plan = (ctypes.c_int * 4)()
    nat.check(L.fpc_conv2d_plan(B, H, W, Cin, Cout, 3, 3, 0, 0, code, plan), "plan")
    out = torch.full((B, H, W, Cout), float("nan"), device=dev)
    gpart = torch.full((B, plan[3], Cout, 2), float("nan"), device=dev) if gn else None
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, H, W, Cin, Cout, 3, 3), dtype=torch.uint8, device=dev)
    sb, sh, sw, sc = xd.stride()
    nat.check(L.fpc_conv2d(xd.data_ptr(), sb, sh, sw, sc, wd.data_ptr(), nat.ptr(scale), nat.ptr(shift), nat.ptr(res), None,
                           out.data_ptr(), nat.ptr(gpart), B, H, W, Cin, Cout, 3, 3, 1, 1, int(relu), 0, 0, code, ws.data_ptr(),
                           ws.numel(), nat.stream()), "conv2d")
    torch.cuda.synchronize()
    return out, gpart


def _launch_is_xshared(nat, H, W, B, Cin, code):
    """what the launcher does with the request: (packed or transposed, on the x-shared map)"""
    L = nat.lib()
    o = (ctypes.c_int64 * 9)()
    if code == ORIENT:
        nat.check(L.fpc_wino_orient_geometry(H, W, B, Cin, 0, 0, o), "geometry")
        tr, G = bool(o[0]), int(o[1])
    else:
        nat.check(L.fpc_wino_pack_geometry(H, W, B, Cin, 0, o), "geometry")
        tr, G = False, int(o[0])
    packed = tr or G > 1
    return packed, packed and bool(L.fpc_wino_xshare_rule(H if tr else W))


def _compare(nat, dev, H, W, B, seed):
    g = torch.Generator().manual_seed(seed)
    ref64_done = False
    taken = set()
    for Cin in CINS:
        x = torch.randn((B, H, W, Cin), generator=g).to(dev)
        for Cout in COUTS:
            w = (torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5).to(dev)
            scale, shift = (torch.rand(Cout, generator=g) + 0.5).to(dev), torch.randn(Cout, generator=g).to(dev)
            res = torch.randn((B, H, W, Cout), generator=g).to(dev)
            for ep in EPILOGUES:
                kw = dict(scale=scale, shift=shift, res=res, relu=True) if ep == "bn_res_relu" else dict(gn=ep == "gn")
                for code, old in ((PACKED, PACKED_ROWSPLIT), (ORIENT, ORIENT_ROWSPLIT)):
                    new_o, new_g = _conv(nat, dev, x, w, code, **kw)
                    old_o, old_g = _conv(nat, dev, x, w, old, **kw)
                    assert not torch.isnan(new_o).any(), "unwritten outputs"
                    assert torch.equal(new_o, old_o), (Cin, Cout, ep, code)
                    if ep == "gn":
                        assert not torch.isnan(new_g).any(), "an unwritten GroupNorm record"
                        assert torch.equal(new_g, old_g), (Cin, Cout, ep, code)
                    taken.add((code,) + _launch_is_xshared(nat, H, W, B, Cin, code))
            if not ref64_done:      # once per shape: the values themselves, against float64 at the bar of every convolution form
                ref64_done = True
                got, _ = _conv(nat, dev, x, w, ORIENT)
                ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), padding=1)
                err = (got.permute(0, 3, 1, 2).cpu().double() - ref).abs().max().item()
                print(f"{H}x{W} B={B}: float64 error {err:.3g} of scale {ref.abs().max().item():.3g}")
                assert err <= 2e-5 * max(1.0, ref.abs().max().item())
    return taken


@pytest.mark.parametrize("H,W,B", SHAPES, ids=lambda v: str(v))
def test_xshared_launch_equals_the_rowsplit_launch(nat, dev, H, W, B):
    taken = _compare(nat, dev, H, W, B, seed=1000 * H + 10 * W + B)
    print("requests (code, packed, x-shared):", sorted(taken))
    if (H, W) != (16, 16):      # every other shape here runs packed AND x-shared under at least one of the two requests
        assert any(xs for _, _, xs in taken), taken


@pytest.mark.parametrize("H,W,B", [(22, 30, 3), (12, 18, 4)], ids=lambda v: str(v))
def test_odd_tile_column_count_keeps_the_rowsplit_map(nat, dev, H, W, B):
    """15 tile columns (22 x 30: nothing packs at this batch either) and 9 (12 x 18: two frames per canvas row, seams after odd counts):
    the rule refuses the x-shared map, the launch is the row-split one and passes the same comparison."""
    assert nat.lib().fpc_wino_xshare_rule(W) == 0
    taken = _compare(nat, dev, H, W, B, seed=7 * H + W)
    assert not any(xs for _, _, xs in taken), taken
    if (H, W) == (12, 18):
        assert (PACKED, True, False) in taken


# ---- the fold (p2 24 x 32 over p3 12 x 16), in both orientations

def _model():
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet34"
    hp.PERFORM_AGGREGATION = False
    torch.manual_seed(0)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    g = torch.Generator().manual_seed(1)
    for name, p in m.named_parameters():      # non-zero lateral biases: the border-class table is exercised
        if name.endswith("p2.skip_conv.bias"):
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return m.eval()


def test_fold_is_bit_identical_on_both_maps_in_both_orientations(nat, dev):
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m = _model().to(dev)
    B, H, W = 3, 96, 128      # p2 24 x 32: transposed, 12 tile columns of the virtual image, two frames per canvas row + a ragged one
    x = torch.stack([synth.make_image(i, H, W) for i in range(B)]).to(dev)
    eng = NetEngine(m, B, H, W, dev, autotune=False, split_precision=3)
    eng.force_winograd(9)
    assert eng.force_fold(1) == 1
    runs = {}
    for orient in (1, 0):
        eng.set_wino_orient(orient)
        for xs in (1, 0):
            eng.set_wino_xshare(xs)
            with torch.no_grad():
                logits, _ = eng.forward(x)
            torch.cuda.synchronize()
            runs[(orient, xs)] = ({k: v.clone() for k, v in logits.items()},
                                  {k: eng.tensor(k).clone() for k in [f"d{d}.seg6" for d in range(4)] + ["c2", "c3", "c4", "c5"]})
    for orient in (1, 0):
        a, b = runs[(orient, 1)], runs[(orient, 0)]
        for part in (0, 1):
            for k in a[part]:
                assert not torch.isnan(a[part][k]).any()
                assert torch.equal(a[part][k], b[part][k]), (orient, k)
