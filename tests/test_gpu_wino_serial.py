"""The serial path of the four-wave Winograd kernels (csrc/wino_tile.hpp: workgroup-id decode, staging set-up, the output transform
image in LDS, the epilogue) may be rearranged freely, but every output element and every GroupNorm record must come out of the same
floating-point operations in the same order.  Three checks on the launches tools_dev/wino_serial_digest.py lists:
  1. the SHA-256 of every output and record tensor equals the one committed in tests/golden/wino_serial_digests.json, which that
     script wrote on the commit before the serial path was last touched (outputs and records start from NaN);
  2. independent of the digests: the same launches against float64 at 2e-5 of the tensor's scale, the records' sums as
     test_gpu_wino_pack.py holds them, and bit-exact on the exact operand grid of test_gpu_conv_operands.py — a digest file written by
     a wrong kernel cannot hide an indexing error;
  3. the folded s2.0 (four decoders as groups) through the engine, in both orientations, digests and float64."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_operands import _assert_bitwise, _exact_case
from test_gpu_p2_fold import _check_seg6

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_tool():
    spec = importlib.util.spec_from_file_location("wino_serial_digest", os.path.join(HERE, "..", "tools_dev", "wino_serial_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tool = _load_tool()
with open(os.path.join(HERE, "golden", "wino_serial_digests.json")) as f:
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
    """[(case, out, records)] of one request, computed once and left unchanged."""
    dev = torch.device("cuda:0")
    return [(case,) + tool.run_case(dev, case) for case in tool.conv_cases(request_)]


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
    conv = {k for k in GOLDEN if not k.startswith("fold-")}
    assert conv == want
    fold = {k for k in GOLDEN if k.startswith("fold-")}
    assert len(fold) == len(tool.FOLD_B) * 2 * (4 + 5) and all(len(v) == 64 for v in GOLDEN.values())


@pytest.mark.parametrize("request_", tool.REQUESTS)
def test_digests_equal_the_commit_before(lib, dev, request_):
    bad = []
    for case, out, gp in _launches(request_):
        assert not torch.isnan(out).any(), (case[0], "unwritten outputs")
        if tool.digest(out) != GOLDEN[case[0] + ":out"]:
            bad.append(case[0] + ":out")
        if gp is not None and tool.digest(gp) != GOLDEN[case[0] + ":records"]:
            bad.append(case[0] + ":records")
    assert not bad, f"{len(bad)} tensors differ from the commit before, the first: {bad[:6]}"


@pytest.mark.parametrize("request_", tool.REQUESTS)
def test_the_same_launches_meet_float64(lib, dev, request_):
    worst = 0.0
    for case, out, gp in _launches(request_):
        name, _, B, Cin, H, W, Cout, epi = case
        _, _, scale, shift, res = tool.operands(B, Cin, H, W, Cout)
        ref = _ref64(B, Cin, H, W, Cout)
        if epi == "bn_relu_res":
            ref = (ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double()).relu()
        got = out.permute(0, 3, 1, 2).double()
        err = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        worst = max(worst, err)
        assert err <= 2e-5, (name, err)
        if gp is not None:
            assert not torch.isnan(gp).any(), (name, "a GroupNorm record the finalize kernel reads was not written")
            s = gp.double().sum(1)      # [B, Cout, 2] over the frame's records, as k_gn_finalize sums
            np.testing.assert_allclose(s[..., 0].numpy(), ref.sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3, err_msg=name)
            np.testing.assert_allclose(s[..., 1].numpy(), (ref * ref).sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3, err_msg=name)
    print("request", request_, "worst float64 error of scale", worst)


# the exact grid: every product and sum exact, so the launch must equal float64 bit for bit whatever the layout of the image in LDS
EXACT_SHAPES = [(3, 23, 31), (3, 24, 32), (2, 40, 24)]


@pytest.mark.parametrize("request_", tool.REQUESTS)
def test_bit_exact_on_the_exact_grid(lib, dev, request_):
    for B, H, W in EXACT_SHAPES:
        for Cout in tool.COUTS:
            shape = (B, 32 if request_ <= -9 else 16, H, W, Cout, 3, 1, 1)
            x, w, kw, ref = _exact_case(shape, "wino", 0)
            out, _ = tool.run_conv(dev, request_, x, w, scale=kw["scale"], shift=kw["shift"], relu=kw["relu"])
            _assert_bitwise(out.permute(0, 3, 1, 2), ref, f"request {request_} on {shape}")


@pytest.mark.parametrize("B", tool.FOLD_B)
def test_fold_digests_and_float64(lib, dev, B):
    built = tool.fold_engine(dev, B)
    bad = []
    for orient in (1, 0):
        got = tool.run_fold(dev, B, orient, built)
        bad += [k for k, v in got.items() if tool.digest(v) != GOLDEN[k]]
        _check_seg6(built[0], built[1], list(range(B)))
    assert not bad, bad
