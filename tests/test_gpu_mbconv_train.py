"""The gradients of the EfficientNet-B0 encoder's depthwise convolution on the native kernels (csrc/depthwise.hip), through the C
ABI: fpc_mbconv_dw_dgrad / _wgrad against the float64 references of _mbconv_train_refs (which tests/test_mbconv_train_host.py shows to
be float64 autograd).  Bars: dx within 2e-5 max(1, |ref|max) of float64, dw within 1e-4 max(1, |ref|max); outputs in NaN-filled
buffers between 64-float canaries, every launch twice and bit-identical."""
import pytest
import torch

import _mbconv_train_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    """The loaded library: a missing one fails here, once, not in every case."""
    from fastposecnn_amd import _native
    return _native.lib()


def _twice(dev, n, launch):
    """Two launches into fresh NaN-filled buffers with 64-float canaries around the n outputs: the canaries intact, nothing left
    unwritten, both runs the same bits.  Returns the first run's outputs (CPU, flat)."""
    outs = []
    for _ in range(2):
        buf = torch.full((n + 128,), float("nan"), device=dev)
        y = buf[64:64 + n]
        assert y.data_ptr() % 16 == 0
        assert launch(y.data_ptr()) == 0
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.isnan(host[:64]).all() and torch.isnan(host[64 + n:]).all(), "a canary was overwritten"
        outs.append(host[64:64 + n])
    assert not torch.isnan(outs[0]).any(), "unwritten outputs"
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def _bar(out, ref, what, rel):
    err = (out.detach().double().cpu() - ref).abs().max().item()
    bar = rel * max(1.0, ref.abs().max().item())
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar, (what, err, bar)


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _dgrad(dev, shape, k, s, dy, w, entry="mb"):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, Hi, Wi, C = shape
    dyd, wd = _nhwc(dy, dev), w.to(dev)
    if entry == "mb":
        call = lambda p: L.fpc_mbconv_dw_dgrad(dyd.data_ptr(), wd.data_ptr(), p, B, Hi, Wi, C, k, s, nat.stream())
    else:
        call = lambda p: L.fpc_dwconv3x3_dgrad(dyd.data_ptr(), wd.data_ptr(), p, B, Hi, Wi, C, s, nat.stream())
    return _twice(dev, B * Hi * Wi * C, call).view(B, Hi, Wi, C).permute(0, 3, 1, 2)


def _wgrad(dev, shape, k, s, x, dy, entry="mb"):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, Hi, Wi, C = shape
    Ho, Wo = Hi // s, Wi // s
    xd, dyd = _nhwc(x, dev), _nhwc(dy, dev)
    need = L.fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, k)
    assert need == R.wgrad_slices(B, Ho, Wo, C, k) * C * k * k * 4
    ws = torch.full((need // 4 + 64,), float("nan"), device=dev)      # (the partials are all written before they are read)
    assert ws.data_ptr() % 256 == 0
    if entry == "mb":
        call = lambda p: L.fpc_mbconv_dw_wgrad(xd.data_ptr(), dyd.data_ptr(), p, B, Hi, Wi, C, k, s, ws.data_ptr(), need, nat.stream())
    else:
        call = lambda p: L.fpc_dwconv3x3_wgrad(xd.data_ptr(), dyd.data_ptr(), p, B, Hi, Wi, C, s, ws.data_ptr(), need, nat.stream())
    out = _twice(dev, C * k * k, call)
    assert torch.isnan(ws[need // 4:]).all(), "the workspace was written past its size"
    return out.view(C, 1, k, k)


# ---- the kernels through the C ABI --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES_ALL, ids=R.ids(R.SHAPES_ALL))
@pytest.mark.parametrize("ks", R.KS, ids=["k%ds%d" % ks for ks in R.KS])
def test_gradients_vs_float64(lib, dev, ks, shape):
    """Both gradients at the bars, then on whole numbers in [-4, 4] — every product and partial sum exact in f32 — bit for bit
    against float64: a window one cell off does not survive that.  The two extra shapes are for the weight gradient alone."""
    k, s = ks
    B, Hi, Wi, C = shape
    if shape == R.WGRAD_EXTRA[0]:
        assert R.wgrad_slices(B, Hi // s, Wi // s, C, k) > 1
    if shape == R.WGRAD_EXTRA[1]:
        assert B * (Hi // s) * ((Wi // s + 7) // 8) < 8
    for integer in (False, True):
        x, w, dy = R.operands(shape, k, s, integer)
        if shape in R.SHAPES:
            dx, ref = _dgrad(dev, shape, k, s, dy, w), R.dgrad_ref(dy, w, Hi, Wi, k, s)
            if integer:
                assert torch.equal(dx.double(), ref), "dx on whole numbers"
            else:
                _bar(dx, ref, f"dgrad {ks} {shape}", 2e-5)
        dw, ref = _wgrad(dev, shape, k, s, x, dy), R.wgrad_ref(x, dy, k, s)
        if integer:
            assert torch.equal(dw.double(), ref), "dw on whole numbers"
        else:
            _bar(dw, ref, f"wgrad {ks} {shape}", 1e-4)


@pytest.mark.parametrize("C", [4, 40])
def test_unreached_taps_are_exact_zeros_and_channels_do_not_mix(lib, dev, C):
    """The (2, 2, 2, C) map at k = 5, stride 1: of the 25 taps only the inner 3 x 3 meets a pixel, the other 16 are exact zeros;
    dy in one channel only leaves every other channel of dx and dw exactly zero."""
    shape, k, s = (2, 2, 2, C), 5, 1
    g = torch.Generator().manual_seed(77 + C)
    x, w, dy = torch.randn((2, C, 2, 2), generator=g), torch.randn((C, 1, 5, 5), generator=g), torch.randn((2, C, 2, 2), generator=g)
    dw = _wgrad(dev, shape, k, s, x, dy).view(C, 5, 5)
    reached = torch.zeros((5, 5), dtype=torch.bool)
    reached[1:4, 1:4] = True
    assert (dw[:, ~reached] == 0).all() and (dw[:, reached] != 0).all()
    _bar(dw.reshape(C, 1, 5, 5), R.wgrad_ref(x, dy, k, s), "dw", 1e-4)
    ch = C // 2 + 1
    one = torch.zeros_like(dy)
    one[:, ch] = dy[:, ch]
    other = torch.ones(C, dtype=torch.bool)
    other[ch] = False
    dx, dw = _dgrad(dev, shape, k, s, one, w), _wgrad(dev, shape, k, s, x, one)
    _bar(dx, R.dgrad_ref(one, w, 2, 2, k, s), "dx, one channel", 2e-5)
    _bar(dw, R.wgrad_ref(x, one, k, s), "dw, one channel", 1e-4)
    assert (dx[:, other] == 0).all() and (dx[:, ch] != 0).any()
    assert (dw[other] == 0).all() and (dw[ch] != 0).any()


@pytest.mark.parametrize("shape", [(1, 6, 10, 32), (2, 22, 80, 8), (3, 30, 40, 144)], ids=str)
def test_k3_stride1_is_the_pad1_kernels_bit_for_bit(lib, dev, shape):
    B, Hi, Wi, C = shape
    x, w, dy = R.operands(shape, 3, 1)
    assert torch.equal(_dgrad(dev, shape, 3, 1, dy, w), _dgrad(dev, shape, 3, 1, dy, w, entry="dw3x3"))
    assert torch.equal(_wgrad(dev, shape, 3, 1, x, dy), _wgrad(dev, shape, 3, 1, x, dy, entry="dw3x3"))
