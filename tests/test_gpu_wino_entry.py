"""The entry of k_conv_wino_h3 (csrc/wino_h3.hip): the accumulators start from +0.0 written by sixteen matrix instructions on zero
operands, and the staged input ring reads zero wherever no LDS-DMA piece writes (wino_zero_ring).

Stale accumulators.  Accumulator registers are not cleared between workgroups: a missed zero shows as a leftover of an earlier
launch.  Every case runs once (`clean`), then again behind launches on operands of scale 1e3 under requests -9, -11 and -13 that
fill every CU; the second run must EQUAL the first, and both meet float64 at the 2e-5 bar of every convolution form.

Seams and borders.  Packed launches on both tile maps (x-shared -10 / -11 against row-split -12 / -13) over frames of 2, 6, 10 and 12
tile columns, B = 3 and 5, odd and even sizes, transposed and not, against each other (equal) and against float64.  A host check
through the kernels' own decode (fpc_wino_tile_patch) holds that these shapes produce every class of wino_zero_ring's condition —
top, left, bottom, right, seam, interior — and seams after 2, 4 and 6 tile columns beside patches without one.  (A seam after 0
columns is not a decode result: a patch starts inside its frame, so at least one tile column lies in front of the seam.)"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PLAIN, PACKED, ORIENT, PACKED_ROWSPLIT, ORIENT_ROWSPLIT = -9, -10, -11, -12, -13
DEC = ("mask_decoder", "rotation_decoder", "translation_decoder", "scales_decoder")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat(dev):
    from fastposecnn_amd import _native
    _native.lib()
    return _native


def _conv(nat, dev, xd, wd, code, gn=False):
    L = nat.lib()
    B, H, W, Cin = xd.shape
    Cout = wd.shape[0]
    plan = (ctypes.c_int * 4)()
    nat.check(L.fpc_conv2d_plan(B, H, W, Cin, Cout, 3, 3, 0, 0, code, plan), "plan")
    out = torch.full((B, H, W, Cout), float("nan"), device=dev)
    gpart = torch.full((B, plan[3], Cout, 2), float("nan"), device=dev) if gn else None
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, H, W, Cin, Cout, 3, 3), dtype=torch.uint8, device=dev)
    sb, sh, sw, sc = xd.stride()
    nat.check(L.fpc_conv2d(xd.data_ptr(), sb, sh, sw, sc, wd.data_ptr(), None, None, None, None, out.data_ptr(), nat.ptr(gpart),
                           B, H, W, Cin, Cout, 3, 3, 1, 1, 0, 0, 0, code, ws.data_ptr(), ws.numel(), nat.stream()), "conv2d")
    torch.cuda.synchronize()
    return out, gpart


def _ref64(x, w):
    return F.conv2d(x.permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), padding=1).permute(0, 2, 3, 1)


def _meets_float64(got, ref, what):
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (what, err, ref.abs().max().item())


_DIRTY = []      # the dirtying launches' operands, made once


def _dirty(nat, dev):
    """Launches whose accumulators end far from zero on every CU: operands of scale 1e3 (sums of the order of 1e6 and more), 360
    workgroups and more per launch, under the plain, the transposed x-shared and the transposed row-split request."""
    if not _DIRTY:
        g = torch.Generator().manual_seed(99)
        _DIRTY.append((torch.randn((8, 60, 96, 16), generator=g) * 1e3).to(dev))      # 30 x 48 tiles: transposed under -11 / -13
        _DIRTY.append((torch.randn((128, 16, 3, 3), generator=g) * 1e3).to(dev))
    x, w = _DIRTY
    for code in (PLAIN, ORIENT, ORIENT_ROWSPLIT):
        out, _ = _conv(nat, dev, x, w, code)
        assert torch.isfinite(out).all() and out.abs().max().item() > 1e5


STALE_CASES = [(B, H, W) for B in (2, 3) for (H, W) in ((24, 32), (23, 31))]


@pytest.mark.parametrize("B,H,W", STALE_CASES, ids=lambda v: str(v))
def test_no_leftover_of_an_earlier_launch_in_the_accumulators(nat, dev, B, H, W):
    g = torch.Generator().manual_seed(100 * H + B)
    cases = []
    for Cin in (16, 48):      # one pair of K-steps (the loop runs once) and three
        x = torch.randn((B, H, W, Cin), generator=g).to(dev)
        for Cout in (64, 128):
            w = (torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5).to(dev)
            cases.append((x, w, _ref64(x, w)))
    runs = [(x, w, ref, code, gn) for (x, w, ref) in cases for code in (PLAIN, ORIENT, ORIENT_ROWSPLIT) for gn in (False, True)]
    clean = [_conv(nat, dev, x, w, code, gn=gn) for (x, w, ref, code, gn) in runs]
    _dirty(nat, dev)
    for (x, w, ref, code, gn), (out0, rec0) in zip(runs, clean):
        what = (tuple(x.shape), w.shape[0], code, gn)
        out1, rec1 = _conv(nat, dev, x, w, code, gn=gn)
        assert not torch.isnan(out1).any(), what
        assert torch.equal(out1, out0), what
        if gn:
            assert not torch.isnan(rec1).any(), what
            assert torch.equal(rec1, rec0), what
        _meets_float64(out0, ref, what)
        _meets_float64(out1, ref, what)


# ---- the fold: phase 2 zeroes nothing and keeps phase 1's sums

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


def _seg6_ref(m, eng, d):
    """float64 conv3x3(W, L c2 + b + up2(p3)) from the engine's own c2 and p3: the UNFOLDED computation (test_gpu_p2_fold.py)"""
    sd = dict(m.named_parameters())
    Lw = sd[f"{DEC[d]}.p2.skip_conv.weight"].detach().cpu().double()
    b = sd[f"{DEC[d]}.p2.skip_conv.bias"].detach().cpu().double()
    Wt = sd[f"{DEC[d]}.seg_blocks.3.block.0.block.0.weight"].detach().cpu().double()
    c2 = eng.tensor("c2").detach().cpu().double().permute(0, 3, 1, 2)
    p3 = eng.tensor(f"d{d}.p3").detach().cpu().double().permute(0, 3, 1, 2)
    return F.conv2d(F.conv2d(c2, Lw, b) + F.interpolate(p3, scale_factor=2, mode="nearest"), Wt, padding=1)


def test_fold_keeps_phase_one_sums_behind_a_dirty_launch(nat, dev):
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    m = _model().to(dev)
    B, H, W = 3, 96, 128      # p2 24 x 32
    x = torch.stack([synth.make_image(i, H, W) for i in range(B)]).to(dev)
    eng = NetEngine(m, B, H, W, dev, autotune=False, split_precision=3)
    eng.force_winograd(9)
    assert eng.force_fold(1) == 1
    names = [f"d{d}.seg6" for d in range(4)]

    def forward():
        with torch.no_grad():
            eng.forward(x)
        torch.cuda.synchronize()
        return {k: eng.tensor(k).clone() for k in names}

    refs = None
    for orient in (1, 0):
        eng.set_wino_orient(orient)
        for idle in (1, 0):      # all_rows = 0 / 1
            eng.set_fold_idle_row(idle)
            first = forward()
            if refs is None:      # (c2 and p3 do not depend on the two switches)
                refs = [_seg6_ref(m, eng, d) for d in range(4)]
            _dirty(nat, dev)
            again = forward()
            for d, k in enumerate(names):
                assert not torch.isnan(again[k]).any(), (orient, idle, k)
                assert torch.equal(again[k], first[k]), (orient, idle, k)
                got = again[k].cpu().double().permute(0, 3, 1, 2)
                err = (got - refs[d]).abs().max().item() / refs[d].abs().max().item()
                assert err <= 2e-5, (orient, idle, k, err)


# ---- seams and borders

# stored orientation (-10 / -12): 2, 6, 10 and 12 tile columns, even and odd H and W (17, 18 rows: two patch rows, the lower one cut);
# transposed (-11 / -13: tile columns a multiple of 8, tile rows 10 or 12, which become the virtual image's tile columns), even and
# odd; 52 x 52: four patch rows of which two are interior, patches without a seam between a frame's borders
SEAM_SHAPES = ([(H, W) for W in (4, 12, 20, 24) for H in (18, 17)] + [(18, 19), (17, 23), (18, 3), (17, 11)] +
               [(20, 32), (19, 31), (24, 16), (23, 15)] + [(52, 52)])
SEAM_BATCHES = (3, 5)


def _patch_classes(nat, H, W, B, Cin, code):
    """border classes (wino_zero_ring's condition, term by term) and seam positions of the launch's patches, by the kernels' decode"""
    L = nat.lib()
    o = (ctypes.c_int64 * 9)()
    if code in (ORIENT, ORIENT_ROWSPLIT):
        nat.check(L.fpc_wino_orient_geometry(H, W, B, Cin, 0, 0, o), "geometry")
        tr, G, tbx, tby, patches = bool(o[0]), int(o[1]), int(o[2]), int(o[3]), int(o[4])
        packed = tr
    else:
        nat.check(L.fpc_wino_pack_geometry(H, W, B, Cin, 0, o), "geometry")
        tr, G, tbx, tby, patches = False, int(o[0]), int(o[1]), int(o[2]), int(o[3])
        packed = G > 1
    Hv, Wv = (W, H) if tr else (H, W)
    if not packed:      # the plain launch: one frame per patch row
        tbx, tby = -(-((Wv + 1) // 2) // 8), -(-((Hv + 1) // 2) // 8)
        patches = tbx * tby * B
    classes, seams = set(), set()
    p = (ctypes.c_int64 * 8)()
    for k in range(patches):
        nat.check(L.fpc_wino_tile_patch(int(packed), Hv, Wv, B, tbx, tby, G if packed else 1, k, p), "patch")
        ty0, tx0, ks = int(p[1]), int(p[2]), int(p[3])
        y0, x0 = 2 * ty0 - 1, 2 * tx0 - 1
        c = {n for n, hit in (("top", y0 < 0), ("left", x0 < 0), ("bottom", y0 + 18 > Hv), ("right", x0 + 18 > Wv),
                              ("seam", packed and ks < 8)) if hit}
        classes |= c or {"interior"}
        seams.add(ks if packed and ks < 8 else None)
    return classes, seams, tr, packed


def test_the_seam_shapes_reach_every_border_class_and_seam():
    from fastposecnn_amd import _native as nat
    nat.lib()
    classes, seams, kinds = set(), set(), set()
    for (H, W) in SEAM_SHAPES:
        for B in SEAM_BATCHES:
            for code in (PACKED, ORIENT):
                c, s, tr, packed = _patch_classes(nat, H, W, B, 16, code)
                classes |= c; seams |= s; kinds.add((tr, packed))
    assert classes == {"top", "left", "bottom", "right", "seam", "interior"}, classes
    assert seams >= {2, 4, 6, None}, seams
    assert 0 not in seams      # (see the module's docstring)
    assert {(True, True), (False, True), (False, False)} <= kinds, kinds


@pytest.mark.parametrize("H,W", SEAM_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("B", SEAM_BATCHES)
def test_seam_and_border_patches_on_both_maps(nat, dev, B, H, W):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B)
    Cin, Cout = 16, 64
    x = torch.randn((B, H, W, Cin), generator=g).to(dev)
    w = (torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5).to(dev)
    ref = _ref64(x, w)
    _dirty(nat, dev)      # stale ring contents and accumulators of another launch in front of every pair
    for xs_code, rs_code in ((PACKED, PACKED_ROWSPLIT), (ORIENT, ORIENT_ROWSPLIT)):
        xs_o, xs_g = _conv(nat, dev, x, w, xs_code, gn=True)
        rs_o, rs_g = _conv(nat, dev, x, w, rs_code, gn=True)
        assert not torch.isnan(xs_o).any() and not torch.isnan(xs_g).any(), xs_code
        assert torch.equal(xs_o, rs_o), (xs_code, rs_code)
        assert torch.equal(xs_g, rs_g), (xs_code, rs_code)
        _meets_float64(xs_o, ref, xs_code)
        _meets_float64(rs_o, ref, rs_code)
