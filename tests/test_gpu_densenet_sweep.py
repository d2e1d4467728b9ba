"""The DenseNet kernels (csrc/densenet.hip) at the loop and grid shapes tests/test_gpu_densenet.py leaves out, with its discipline:
float64 torch on the CPU as reference, the kernel bar 2e-5 max(1, |ref|max), every case launched twice and bit-identical, NaN-filled
outputs between 64-float canaries, a pattern wherever a pitched kernel must not write (compared bit for bit), NaN behind channel K of
the input rows, and every case once more on small whole numbers, bit for bit.

  conv3x3   the tile form on a grid rounded up to the XCD bands with waves past the last tile (forced, and as a shape's own form at
            1024 waves), the split form on grids of 16 and 24 workgroups (bands of 2 and 3), one-hot pixels in the ragged last tile
            and on a frame boundary inside a tile
  pw        3, 6, 28 and 56 channel tiles (Cout 96 and 896) under the band permutation, workgroups leaving before the barrier; the
            transition's call (no prologue, no epilogue affine) and each half of it alone; K = 32 (one K-step: the pipeline's loop
            body never runs, three waves of the 16 x 16 form have nothing to sum) and K = 2048, the entry's limits
  norm_pool channel-quad counts that are no power of two (C = 640, 1664, 1920) and one quad

Which grid a case runs on is restated from the launch code (tests/_densenet_kernels.py: conv3_launch, pw_launch) and asserted per
case: a change of the launch arithmetic has to be repeated there, and the cases then say what they no longer cover."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from _densenet_kernels import NAN, _bar, _conv_run, _pitched, _pw_operands, _pw_ref, _twice, conv3_launch, pw_launch

pytestmark = pytest.mark.gpu

SLICES = [(0, 32), (224, 256)]                           # (c0, ldo): dense, and the last slice of a wider pixel
KINDS = ["random", "whole"]


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


# ----------------------------------------------------------------------------------------------------------- fpc_dense_conv3x3

def _conv_operands(B, H, W, whole, seed):
    """Whole numbers: |x| <= 4, |w| <= 3, so every partial sum is at most 1152 x 12 < 2^24 and exact in f32 in any order."""
    g = torch.Generator().manual_seed(seed)
    if whole:
        return torch.randint(-4, 5, (B, 128, H, W), generator=g).float(), torch.randint(-3, 4, (32, 128, 3, 3), generator=g).float()
    return torch.randn((B, 128, H, W), generator=g), torch.randn((32, 128, 3, 3), generator=g) * 2.0 / 1152 ** 0.5


def _conv_check(out, ref, whole, what):
    if whole:
        assert torch.equal(out.double(), ref), what
    else:
        _bar(out, ref, what)


@pytest.mark.parametrize("kind", KINDS)
def test_conv3x3_tile_form_on_a_banded_grid(lib, dev, kind):
    """(3, 27, 29), form 1 forced: 2349 pixels are 37 waves in 10 workgroups, rounded up to 16 — bands of 2 under xcd_block(), 27
    waves past the last tile, which holds 45 of its 64 pixels; a frame is 783 pixels, so tiles straddle frames and rows."""
    from fastposecnn_amd import _native as nat
    B, H, W = 3, 27, 29
    assert conv3_launch(B * H * W, 1) == dict(tiles=37, rows=64, grid=16, band=2, idle=27)
    assert B * H * W - 36 * 64 == 45 and (H * W) % 64 != 0 and W % 32 != 0
    assert nat.lib().fpc_dense_conv3x3_form(B, H, W) == 0                  # (the shape's own form is the other one: forced here)
    x, w = _conv_operands(B, H, W, kind == "whole", 11)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    for c0, ldo in SLICES:
        _conv_check(_conv_run(dev, x, w, c0, ldo, 1), ref, kind == "whole", f"dense_conv3x3 tile {(B, H, W)} c0 {c0}/{ldo} {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_conv3x3_tile_form_as_the_shapes_own(lib, dev, kind):
    """(2, 181, 181): 65 522 pixels, the fewest frames of odd extent with 1024 waves, so form = -1 takes the tile form itself: a grid
    of 256 (bands of 32), no wave past the last tile, which holds 50 pixels.  The forced form's bits."""
    from fastposecnn_amd import _native as nat
    B, H, W = 2, 181, 181
    M = B * H * W
    assert M >= 65473 and nat.lib().fpc_dense_conv3x3_form(B, H, W) == 1 and nat.lib().fpc_dense_conv3x3_form(1, 181, 361) == 0
    assert conv3_launch(M, 1) == dict(tiles=1024, rows=64, grid=256, band=32, idle=0) and M - 1023 * 64 == 50 and (H * W) % 64 != 0
    x, w = _conv_operands(B, H, W, kind == "whole", 12)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    own = _conv_run(dev, x, w, 32, 64, -1)
    _conv_check(own, ref, kind == "whole", f"dense_conv3x3 by shape {(B, H, W)} c0 32/64 {kind}")
    if kind == "random":
        assert torch.equal(own, _conv_run(dev, x, w, 32, 64, 1))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W,grid,band,last", [(1, 11, 23, 16, 2, 13), (3, 16, 8, 24, 3, 16)])
def test_conv3x3_split_form_on_a_permuted_grid(lib, dev, B, H, W, grid, band, last, kind):
    """The split form where xcd_block() is no identity: 253 pixels on 16 workgroups (bands of 2, the last one ragged) and 384 on 24
    (bands of 3, none ragged)."""
    from fastposecnn_amd import _native as nat
    M = B * H * W
    assert conv3_launch(M, 0) == dict(tiles=grid, rows=16, grid=grid, band=band, idle=0) and M - 16 * (grid - 1) == last
    assert nat.lib().fpc_dense_conv3x3_form(B, H, W) == 0
    x, w = _conv_operands(B, H, W, kind == "whole", 13 + H)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    for c0, ldo in SLICES:
        out = _conv_run(dev, x, w, c0, ldo, 0)
        _conv_check(out, ref, kind == "whole", f"dense_conv3x3 split {(B, H, W)} c0 {c0}/{ldo} {kind}")
        assert torch.equal(out, _conv_run(dev, x, w, c0, ldo, -1))          # the shape's own form


@pytest.mark.parametrize("form", [0, 1], ids=["split", "tile"])
def test_conv3x3_one_hot_pixels_in_the_ragged_tile_and_on_a_frame_boundary(lib, dev, form):
    """(3, 27, 29), whole-number weights, two pixels set to 1: the last pixel of the last frame (pixel 2348, in the ragged tile of
    either form) and the first pixel of frame 1 (pixel 783: the tile of 64 from 768 on straddles frames 0 and 1, and so does the
    tile of 16 from 768 on).  Each neighbour at (dh, dw) holds w[n][c][1 - dh][1 - dw] bit for bit and everything else 0: a wrong
    p / W, % H decomposition, or a pad select that looks into the neighbouring frame, cannot hide in a tolerance."""
    B, H, W = 3, 27, 29
    hots = [(2, 101, 26, 28), (1, 7, 0, 0)]                  # (frame, channel, h, w)
    assert (2 * H + 26) * W + 28 == B * H * W - 1 and conv3_launch(B * H * W, 1)["tiles"] == 37 and B * H * W - 1 >= 36 * 64
    assert 768 < 1 * H * W < 768 + 16 and (B * H * W) % 16 != 0
    g = torch.Generator().manual_seed(6)
    w = torch.randint(-9, 10, (32, 128, 3, 3), generator=g).float()
    x = torch.zeros((B, 128, H, W))
    want = torch.zeros((B, 32, H, W))
    for b, c, h0, w0 in hots:
        x[b, c, h0, w0] = 1.0
        for dh in (-1, 0, 1):
            for dw in (-1, 0, 1):
                if 0 <= h0 + dh < H and 0 <= w0 + dw < W:
                    want[b, :, h0 + dh, w0 + dw] = w[:, c, 1 - dh, 1 - dw]
    assert want[0].abs().max() == 0 and want[1, :, 2:].abs().max() == 0 and want[2, :, :25].abs().max() == 0
    out = _conv_run(dev, x, w, 64, 256, form)
    assert torch.equal(out, want)
    assert torch.equal(out.double(), F.conv2d(x.double(), w.double(), None, 1, 1))


# ---------------------------------------------------------------------------------------------------------------- fpc_dense_pw

ALL8 = list(itertools.product((0, 1), (0, 1), (0, 1)))      # (pre, affine, act)


def _pw_case(dev, M, K, ldi, Cout, ldos, combos, whole, seed):
    """Both forms (forced), every output pitch of `ldos`, every (pre, affine, act) of `combos`: pre = s1 / t1 given, affine = s2 / t2
    given.  Whole numbers: |x| <= 4, s1 <= 2, |t1| <= 3, so pre(v) <= 11; |w| <= 2: every partial sum is at most K x 11 x 2
    (45 056 at K = 2048) and the epilogue's 3 x 45 056 + 5 — all below 2^24, so f32 is exact whatever the summation order."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    assert K * 11 * 2 * 3 + 5 < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    x, xin, s1, t1, w, s2, t2 = _pw_operands(g, M, K, ldi, whole, rows=Cout)
    xd, s1d, t1d, wd, s2d, t2d = (t.to(dev) for t in (xin, s1, t1, w, s2, t2))
    for pre, aff, act in combos:
        ref = _pw_ref(x, s1, t1, w, s2, t2, Cout, pre, act, affine=aff)
        for ldo, form in itertools.product(ldos, (0, 1)):
            out = _twice(dev, _pitched(M, ldo, 0, Cout), lambda y: L.fpc_dense_pw(
                xd.data_ptr(), s1d.data_ptr() if pre else None, t1d.data_ptr() if pre else None, wd.data_ptr(),
                s2d.data_ptr() if aff else None, t2d.data_ptr() if aff else None, y, M, K, Cout, ldi, ldo, act, form,
                nat.stream())).view(M, ldo)[:, :Cout]
            assert torch.isfinite(out).all(), "read behind channel K"
            what = f"dense_pw M{M} K{K}/{ldi} Cout{Cout}/{ldo} pre{pre} aff{aff} act{act} form{form} {'whole' if whole else 'random'}"
            if whole:
                assert torch.equal(out.double(), ref), what
            else:
                _bar(out, ref, what)
                if act:
                    assert out.min() >= 0.0
                else:
                    assert out.min() < 0.0              # nothing is clamped


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,K,ldi,Cout,wide", [(333, 160, 512, 96, 256), (45, 1792, 1792, 896, 1024)])
def test_pw_odd_channel_tile_counts(lib, dev, M, K, ldi, Cout, wide, kind):
    """Channel-tile counts that are no power of two, on grids the band permutation reorders: wid % ntiles and wid / ntiles with
    ntiles 3 and 6 (Cout 96) and 28 and 56 (Cout 896, densenet201's third transition's K and Cout).
      M 333, Cout 96:  form 1 — 11 x 3 = 33 waves in 9 workgroups, rounded up to 16 (bands of 2, 31 waves leave at once);
                       form 0 — 21 x 6 = 126 workgroups, rounded up to 128 (bands of 16): two whole workgroups leave before the barrier
      M 45, Cout 896:  form 1 — 2 x 28 = 56 waves in 14 workgroups, rounded up to 16 (bands of 2);
                       form 0 — 3 x 56 = 168 workgroups exactly (bands of 21)"""
    want = {(96, 1): dict(mtiles=11, ntiles=3, waves=33, grid=16, band=2, idle=31),
            (96, 0): dict(mtiles=21, ntiles=6, waves=126, grid=128, band=16, idle=2),
            (896, 1): dict(mtiles=2, ntiles=28, waves=56, grid=16, band=2, idle=8),
            (896, 0): dict(mtiles=3, ntiles=56, waves=168, grid=168, band=21, idle=0)}
    for form in (0, 1):
        assert pw_launch(M, Cout, form) == want[(Cout, form)]
    _pw_case(dev, M, K, ldi, Cout, (Cout, wide), [(0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)], kind == "whole", M + K)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,K,Cout,wide", [(300, 256, 128, 512), (45, 1792, 896, 1024)])
def test_pw_the_transitions_call(lib, dev, M, K, Cout, wide, kind):
    """s1 = t1 = s2 = t2 = NULL, act 0: out = x w^T, what a transition asks (the engine alone reached this arm, at the network bar);
    then the prologue with no epilogue affine, and the epilogue affine with no prologue.  Both forms, a dense and a pitched output."""
    _pw_case(dev, M, K, K, Cout, (Cout, wide), [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 1, 0)], kind == "whole", 3 * M + K)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("K,ldi,Cout,wide", [(32, 32, 64, 256), (32, 256, 64, 256), (2048, 2048, 1024, 1056)])
def test_pw_at_the_limits_of_k(lib, dev, M, K, ldi, Cout, wide, kind):
    """K = 32, the least the entry takes: one K-step, so the two-set pipeline's loop body never runs (only the tail), and on the
    16 x 16 form waves 1 .. 3 have no set and hand over zeros.  K = 2048 and Cout = 1024, the most: 64 K-steps, 16 per wave on the
    16 x 16 form.  One row, and two row tiles with a single row in the second (three on the 16 x 16 form)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    assert L.fpc_dense_pw_form(M, K, Cout) == 0
    assert L.fpc_dense_pw_form(M, K - 32, Cout) == (-1 if K == 32 else 0) and L.fpc_dense_pw_form(M, 2080, Cout) == -1   # the limits
    assert L.fpc_dense_pw_form(M, K, 1056) == -1
    assert pw_launch(M, Cout, 1)["mtiles"] == (1 if M == 1 else 2) and pw_launch(M, Cout, 0)["mtiles"] == (1 if M == 1 else 3)
    _pw_case(dev, M, K, ldi, Cout, (Cout, wide), ALL8, kind == "whole", 5 * M + K + ldi)


# --------------------------------------------------------------------------------------------------------- fpc_dense_norm_pool

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W,C,pool,act", [(2, 6, 10, 1664, True, 0), (2, 6, 10, 1664, True, 1), (1, 30, 40, 640, True, 0),
                                              (1, 30, 40, 640, True, 1), (1, 5, 3, 1920, False, 0), (1, 2, 2, 4, True, 0),
                                              (1, 2, 2, 4, True, 1)])
def test_norm_pool_channel_quads_no_power_of_two(lib, dev, B, H, W, C, pool, act, kind):
    """C / 4 = 416, 160 and 480 channel quads (densenet169's c5, a transition of 640 channels, densenet201's c5): i % CQ and i / CQ
    where a mask and a shift would not do; odd H and W without a pooled tensor; one quad.  test_gpu_densenet.py's layout: skip and
    pooled in ONE canaried buffer with a pattern between them, the pooled tensor 0.25 ((a + b) + (c + d)) of skip bit for bit."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    CQ = C // 4
    assert CQ == 1 or CQ & (CQ - 1), "a power of two: test_gpu_densenet.py's cases"
    g = torch.Generator().manual_seed(H * W + C + act)
    if kind == "whole":        # |s x + t| <= 2 x 8 + 5: exact, and so is a quarter of a sum of four
        x = torch.randint(-8, 9, (B, H, W, C), generator=g).float()
        s, t = torch.randint(1, 3, (C,), generator=g).float(), torch.randint(-5, 6, (C,), generator=g).float()
    else:
        x = torch.randn((B, H, W, C), generator=g)
        s, t = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    ref = x.double() * s.double() + t.double()
    assert ref.min() < 0
    if act:
        ref = ref.clamp_min(0.0)
    xd, sd, td = x.to(dev), s.to(dev), t.to(dev)
    n, npool = x.numel(), x.numel() // 4 if pool else 0
    pre = torch.full((n + 64 + npool,), NAN)
    pre[n:n + 64] = torch.arange(64).float()
    body = _twice(dev, pre, lambda y: L.fpc_dense_norm_pool(xd.data_ptr(), sd.data_ptr(), td.data_ptr(), y, y + 4 * (n + 64) if pool else None,
                                                            B, H, W, C, act, nat.stream()))
    skip = body[:n].view(B, H, W, C)
    what = f"dense_norm_pool {(B, H, W, C)} act{act} {kind}"
    if kind == "whole":
        assert torch.equal(skip.double(), ref), what
    else:
        _bar(skip, ref, what)
    assert (skip.min() >= 0.0) if act else (skip.min() < 0.0)
    if pool:
        pooled = body[n + 64:].view(B, H // 2, W // 2, C)
        want = 0.25 * ((skip[:, 0::2, 0::2] + skip[:, 0::2, 1::2]) + (skip[:, 1::2, 0::2] + skip[:, 1::2, 1::2]))      # f32, the stated order
        assert torch.equal(pooled, want)
        if kind == "whole":
            assert torch.equal(pooled.double(), F.avg_pool2d(ref.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
