"""The two exits of the four-wave Winograd kernels (csrc/wino_tile.hpp: wino_output).  A workgroup whose patch lies wholly inside its
frame leaves through the fast exit — no test of a pixel, the epilogue's parts chosen once —, every other through the general one; both
address their quads from one base and uniform strides.  Every output element and every GroupNorm record must come out of the same
floating-point operations in the same order as before the exits were parted.  On the launches tools_dev/wino_exit_digest.py lists
(every patch inside; one partial row or column of patches; a transposed launch; even and odd tile-column counts; a ragged last canvas
row whose seam patch has no second frame), outputs and records pre-filled with NaN:
  1. the default launch EQUALS (torch.equal) the launch with every workgroup on the general exit (fpc_conv2d's -100 + request,
     fpc_net_set_wino_fast_exit);
  2. the SHA-256 of every tensor equals the one committed in tests/golden/wino_exit_digests.json, which that script wrote on the
     commit before;
  3. independent of both: the same launches against float64 at 2e-5 of the tensor's scale, the bar of these forms;
  4. the folded s2.0 at p2 = 24 x 32 and 32 x 32, B = 2, 3, in both orientations through the engine, the switch both ways."""
import functools
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_p2_fold import _check_seg6

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_tool():
    spec = importlib.util.spec_from_file_location("wino_exit_digest", os.path.join(HERE, "..", "tools_dev", "wino_exit_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tool = _load_tool()
with open(os.path.join(HERE, "golden", "wino_exit_digests.json")) as f:
    GOLDEN = json.load(f)


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


@functools.lru_cache(maxsize=None)
def _launches(request_):
    """[(case, out, records, out of the general exit, its records)] of one request, computed once and left unchanged."""
    dev = torch.device("cuda:0")
    return [(case,) + tool.run_case(dev, case) + tool.run_case(dev, case, general=True) for case in tool.conv_cases(request_)]


@functools.lru_cache(maxsize=None)
def _ref64(B, Cin, H, W, Cout):
    x, w, _, _, _ = tool.operands(B, Cin, H, W, Cout)
    return F.conv2d(x.double(), w.double(), padding=1)


def test_the_golden_file_names_exactly_the_listed_launches():
    want = set()
    for r in tool.REQUESTS:
        for case in tool.conv_cases(r):
            want.add(case[0] + ":out")
            if case[7] == "gn":
                want.add(case[0] + ":records")
    assert {k for k in GOLDEN if not k.startswith("fold-")} == want
    fold = {k for k in GOLDEN if k.startswith("fold-")}
    assert len(fold) == len(tool.FOLD_HW) * len(tool.FOLD_B) * 2 * (4 + 5) and all(len(v) == 64 for v in GOLDEN.values())


def test_the_shapes_walk_both_exits():
    """by the host view of the decode (fpc_wino_tile_patch): the list holds launches of fast patches only and launches of both
    kinds, and seam patches of either kind"""
    import ctypes
    from fastposecnn_amd import _native
    L = _native.lib()
    g8, o8 = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
    kinds, seams = set(), set()
    for B, H, W in tool.SHAPES:
        assert L.fpc_wino_pack_geometry(H, W, B, tool.CIN, 0, g8) == 0
        G, tbx, tby, patches = (int(g8[i]) for i in range(4))
        fast = set()
        for p in range(patches):
            assert L.fpc_wino_tile_patch(1, H, W, B, tbx, tby, G, p, o8) == 0
            fast.add(int(o8[7]))
            if o8[3] < 8:
                seams.add((int(o8[4]), int(o8[7])))
        kinds.add(frozenset(fast))
    assert {frozenset({1}), frozenset({0, 1})} <= kinds, kinds
    assert {(1, 1), (0, 0)} <= seams, seams


@pytest.mark.parametrize("request_", tool.REQUESTS)
def test_fast_exit_equals_general_exit(lib, dev, request_):
    for case, out, gp, out_g, gp_g in _launches(request_):
        assert not torch.isnan(out).any() and not torch.isnan(out_g).any(), (case[0], "unwritten outputs")
        assert torch.equal(out, out_g), case[0]
        if gp is not None:
            assert not torch.isnan(gp).any() and not torch.isnan(gp_g).any(), (case[0], "an unwritten GroupNorm record")
            assert torch.equal(gp, gp_g), case[0]


@pytest.mark.parametrize("request_", tool.REQUESTS)
def test_digests_equal_the_commit_before(lib, dev, request_):
    bad = []
    for case, out, gp, _, _ in _launches(request_):
        if tool.digest(out) != GOLDEN[case[0] + ":out"]:
            bad.append(case[0] + ":out")
        if gp is not None and tool.digest(gp) != GOLDEN[case[0] + ":records"]:
            bad.append(case[0] + ":records")
    assert not bad, f"{len(bad)} tensors differ from the commit before, the first: {bad[:6]}"


@pytest.mark.parametrize("request_", tool.REQUESTS)
def test_the_same_launches_meet_float64(lib, dev, request_):
    worst = 0.0
    for case, out, gp, out_g, _ in _launches(request_):
        name, _, B, Cin, H, W, Cout, epi = case
        _, _, scale, shift, res = tool.operands(B, Cin, H, W, Cout)
        ref = _ref64(B, Cin, H, W, Cout)
        if epi == "bn_relu_res":
            ref = (ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double()).relu()
        for got in (out, out_g):
            err = (got.permute(0, 3, 1, 2).double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
            worst = max(worst, err)
            assert err <= 2e-5, (name, err)
        if gp is not None:
            s = gp.double().sum(1)      # [B, Cout, 2] over the frame's records, as k_gn_finalize sums
            torch.testing.assert_close(s[..., 0], ref.sum((2, 3)), rtol=1e-4, atol=1e-3, msg=name)
            torch.testing.assert_close(s[..., 1], (ref * ref).sum((2, 3)), rtol=1e-4, atol=1e-3, msg=name)
    print("request", request_, "worst float64 error of scale", worst)


@pytest.mark.parametrize("B", tool.FOLD_B)
@pytest.mark.parametrize("hw", tool.FOLD_HW, ids=lambda v: f"{v[0]}x{v[1]}")
def test_fold_on_both_exits(lib, dev, hw, B):
    built = tool.fold_engine(dev, B, hw)
    bad = []
    for orient in (1, 0):
        built[1].set_wino_fast_exit(1)
        got = tool.run_fold(dev, B, hw, orient, built)
        _check_seg6(built[0], built[1], list(range(B)))
        built[1].set_wino_fast_exit(0)
        gen = tool.run_fold(dev, B, hw, orient, built)
        for k, v in got.items():
            assert not torch.isnan(v).any(), k
            assert torch.equal(v, gen[k]), (k, "the two exits differ")
        bad += [k for k, v in got.items() if tool.digest(v) != GOLDEN[k]]
    assert not bad, bad
