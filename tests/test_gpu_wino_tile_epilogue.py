"""The output transform and epilogue the four-wave Winograd kernels share (csrc/wino_tile.hpp: wino_output), on operands where it
has no rounding to hide behind.

Operands: the tier-0 grid of tests/test_gpu_conv_operands.py (x multiples of 2^-4 in [-2, 2], w multiples of 2^-4 in [-1, 1]): every
product and every partial sum of every form is exact, so the convolution is a multiple of 2^-8 that float64 gives exactly.  On top: a
power-of-two scale (2^-1 .. 2^1), an integer shift, an integer residual and ReLU — each step stays on the grid 2^-9 below 2^14
(asserted), so forms -7, -8 and -9 must give float64's bits and each other's.  They cut the same 8 x 8 tile patches and reduce their
GroupNorm records in the same order, so the records must be equal bit for bit too (their sums of squares are rounded, identically);
against float64 they are held to the tolerance of tests/test_gpu_wino_pack.py.  Form -10 (the packed patch grid) must repeat -9's
outputs bit for bit; its records are another grouping and are held to float64 only.  Outputs and records start from NaN."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_operands import _abs_sum_bound, _assert_bitwise, _exact_case
from test_gpu_wino_pack import _conv, _geometry

pytestmark = pytest.mark.gpu

# B, Cin, H, W, Cout
SHAPES = [
    (2, 16, 18, 34, 64),     # 2 x 3 patches, the last row and column mostly outside the image; one pair of K-steps
    (1, 32, 7, 9, 128),      # odd sizes, a single patch, two channel blocks
    (1, 16, 48, 48, 64),     # the centre patch is interior: the only path that skips the buffer zeroing
    (3, 16, 15, 20, 64),     # -10 packs three frames per canvas row: seams
]
FORMS = (-7, -8, -9, -10)


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


@pytest.mark.parametrize("variant", ["scale_shift_res_relu", "gn"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d-%dx%dx%d-%d" % s)
def test_shared_epilogue_is_exact_and_the_same_in_every_form(lib, dev, shape, variant):
    B, Cin, H, W, Cout = shape
    shape8 = (B, Cin, H, W, Cout, 3, 1, 1)
    x, w = _exact_case(shape8, "wino", 0)[:2]
    g = torch.Generator().manual_seed(7 + H + W)
    full = variant == "scale_shift_res_relu"
    shift = torch.randint(-4, 5, (Cout,), generator=g).float()
    scale = 2.0 ** torch.randint(-1, 2, (Cout,), generator=g).float() if full else None      # the "gn" variant: bias only, as the decoder
    res = torch.randint(-8, 9, (B, Cout, H, W), generator=g).float() if full else None
    # the premise: every partial sum (multiples of 2^-10 in the transform domain) and every epilogue step (multiples of 2^-9) is exact
    worst = _abs_sum_bound("wino", shape8, x, w)
    assert worst * 2.0 ** 10 < 2.0 ** 24 and (2.0 * worst + 12.0) * 2.0 ** 9 < 2.0 ** 24, worst
    ref = F.conv2d(x.double(), w.double(), padding=1)
    if full:
        ref = (ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double()).relu()
    else:
        ref = ref + shift.double().view(1, -1, 1, 1)
    assert torch.equal(ref.float().double(), ref)
    if shape == SHAPES[3]:
        assert _geometry(H, W, B, Cin)["G"] > 1, "the case does not pack"

    xd, wd = x.permute(0, 2, 3, 1).contiguous().to(dev), w.contiguous().to(dev)
    kw = dict(shift=shift.to(dev), relu=full, gn=True)
    if full:
        kw.update(scale=scale.to(dev), res=res.permute(0, 2, 3, 1).contiguous().to(dev))
    outs, recs = {}, {}
    for n in FORMS:
        out, rec, _ = _conv(dev, xd, wd, n, **kw)
        assert not torch.isnan(out).any(), f"form {n}: unwritten outputs"
        assert not torch.isnan(rec).any(), f"form {n}: a GroupNorm record was not written"
        outs[n], recs[n] = out.permute(0, 3, 1, 2).cpu(), rec.cpu()
    for n in (-7, -8, -9):
        _assert_bitwise(outs[n], ref, f"form {n} on {shape}, {variant}")
        assert torch.equal(recs[n], recs[-7]), f"form {n}: GroupNorm records differ from form -7's"
    assert torch.equal(outs[-10], outs[-9]), "the packed launch is not bit-identical to the plain one"
    for n in FORMS:
        s = recs[n].double().sum(1)                                # [B, Cout, 2] over the frame's records, as k_gn_finalize sums
        np.testing.assert_allclose(s[..., 0].numpy(), ref.sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(s[..., 1].numpy(), (ref * ref).sum((2, 3)).numpy(), rtol=1e-4, atol=1e-3)
