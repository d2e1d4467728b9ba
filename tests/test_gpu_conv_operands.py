"""Every convolution form of fpc_conv2d on operands that are NOT iid N(0, 1): exact grids (every form must equal float64 bit for
bit), worst-case mantissas, per-channel scale disparity, weight maxima on a binade edge, scaled weights and scaled activations, and
the network on parameters that are not random-init.  The per-value bound of the fp16 piece pair (tests/test_piece_arithmetic.py:
h2_bound) is propagated through the convolutions in float64 here; the Winograd transforms for that are a numpy F(2x2, 3x3) that
doubles as an independent float64 Winograd reference.

Forms by fpc_conv2d request.  fp16 pieces: -8 (all four products), -9 / -10 (three, plain / packed geometry), 6000 + split and
6100 + split (k_conv_igemm), 7000 + parts (k_lateral1x1), 3100 (stem + max-pool).  Range-free siblings on three bf16 pieces: -7,
1000 + split, 2000 + parts, 3000.  Also -1 .. -4 (f32 Winograd), -5 / -6 (bf16 x 3 Winograd), 4000 + variant (pointwise), and
k_conv_igemm on plain f32 products."""
import copy
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_net import _conv2d, _model
from test_piece_arithmetic import H2_ABS, H2_FULL, H2_SAT, h2_bound, split_bf3, split_h2

pytestmark = pytest.mark.gpu

STEM, STEM_POOL = 3000, 3100


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


# ---- one way to run any form, one float64 reference

# kind: "wino" (3x3 / 1 / 1 through the Winograd transforms), "direct", "lateral", "pw" (the operands themselves), "stem" (7x7 / 2
# on the NHWC4 image; request 3100 returns the max-pooled tensor).  three: the form drops the product of the two second pieces.
Form = namedtuple("Form", "name nsplit bm bn kind three", defaults=(0, 0, "direct", False))
# B, Cin, Hi, Wi, Cout, k, stride, pad
S3A, S3B, S3C = (1, 16, 20, 24, 64, 3, 1, 1), (1, 32, 20, 24, 64, 3, 1, 1), (3, 24, 32, 32, 192, 3, 1, 1)
S3A128, S3C128, S3TINY = (1, 16, 20, 24, 128, 3, 1, 1), (3, 24, 16, 32, 128, 3, 1, 1), (1, 8, 7, 9, 64, 3, 1, 1)
S3B128 = (1, 32, 20, 24, 128, 3, 1, 1)                                   # two K-pairs, ragged border patches, two 64-channel blocks
DIRECT, LATERAL, POINTWISE = (2, 64, 9, 11, 96, 3, 2, 1), (3, 64, 10, 14, 96, 1, 1, 0), (3, 64, 10, 14, 128, 1, 1, 0)
STEM_SHAPE = (2, 3, 96, 128, 64, 7, 2, 3)                                # the smallest frame of test_gpu_stem_pool.py
PACK1, PACK2, PACK2_128 = (3, 16, 15, 20, 64, 3, 1, 1), (4, 32, 9, 17, 64, 3, 1, 1), (4, 32, 9, 17, 128, 3, 1, 1)

F32 = Form("f32", 1, 64, 64)
W7, W8 = Form("-7", -7, kind="wino"), Form("-8", -8, kind="wino")
W9, W10 = Form("-9", -9, kind="wino", three=True), Form("-10", -10, kind="wino", three=True)
BF3, H3 = Form("1001", 1001, 64, 64), Form("6001", 6001, 64, 64, three=True)
LAT_BF3, LAT_H3 = Form("2003", 2003, kind="lateral"), Form("7003", 7003, kind="lateral", three=True)
STEM_BF3, STEM_H3 = Form("3000", STEM, kind="stem"), Form("3100", STEM_POOL, kind="stem", three=True)


def _stem(dev, x, w, nsplit, scale=None, shift=None):
    """x [B,3,H,W], w [64,3,7,7] through the stem kernels (NHWC4 image, ReLU always): [B,64,Ho,Wo], or the pooled tensor for 3100."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, _, Hi, Wi = x.shape
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    x4 = torch.cat([x, torch.zeros(B, 1, Hi, Wi)], 1).permute(0, 2, 3, 1).contiguous().to(dev)
    w4 = torch.cat([w, torch.zeros(64, 1, 7, 7)], 1).contiguous().to(dev)
    sb, sh, sw, sc = x4.stride()
    shape = (B, Ho // 2, Wo // 2, 64) if nsplit == STEM_POOL else (B, Ho, Wo, 64)
    out = torch.full(shape, float("nan"), device=dev)
    nbytes = max(L.fpc_conv2d_workspace_bytes(B, Ho, Wo, 4, 64, 7, 7), L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, 4, 64, 7, 7, 0, 0, nsplit))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    t = lambda a: None if a is None else a.contiguous().to(dev)
    scale_d, shift_d = t(scale), t(shift)
    nat.check(L.fpc_conv2d(x4.data_ptr(), sb, sh, sw, sc, w4.data_ptr(), nat.ptr(scale_d), nat.ptr(shift_d), None, None, out.data_ptr(),
                           None, B, Hi, Wi, 4, 64, 7, 7, 2, 3, 1, 0, 0, nsplit, ws.data_ptr(), ws.numel(), nat.stream()), "conv2d")
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu()


def _run(dev, form, shape, x, w, scale=None, shift=None, relu=False, pool=False):
    """pool: 3000 followed by torch's max-pool, 3100's sibling."""
    stride, pad = shape[6], shape[7]
    if form.kind == "stem":
        out = _stem(dev, x, w, form.nsplit, scale, shift)
        return F.max_pool2d(out, 3, 2, 1) if form.nsplit == STEM and pool else out
    return _conv2d(dev, x, w, stride, pad, scale=scale, shift=shift, relu=relu, bm=form.bm, bn=form.bn, nsplit=form.nsplit)[0]


def _ref(form, shape, x, w, scale=None, shift=None, relu=False, pooled=False):
    """float64.  The stem kernels apply ReLU whatever the request says."""
    y = F.conv2d(x.double(), w.double(), stride=shape[6], padding=shape[7])
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if relu or form.kind == "stem":
        y = y.relu()
    return F.max_pool2d(y, 3, 2, 1) if pooled else y


def _chan_err(out, ref):
    """(max error, max |ref|) per output channel."""
    return (out.double() - ref).abs().amax((0, 2, 3)), ref.abs().amax((0, 2, 3))


# ---- numpy F(2x2, 3x3): the transforms of the Winograd forms in float64

BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def _tiles(x):
    """[B,C,H,W] -> the 4 x 4 input tiles of the 2 x 2 output tiles, pad 1: [B,C,ty,tx,4,4] (a copy)."""
    B, C, H, W = x.shape
    ty, tx = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, C, 2 * ty + 2, 2 * tx + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    s = xp.strides
    return np.lib.stride_tricks.as_strided(xp, (B, C, ty, tx, 4, 4), (s[0], s[1], 2 * s[2], 2 * s[3], s[2], s[3])).copy()


def _wino_v(x, absolute=False):
    m = np.abs(BT) if absolute else BT
    return np.einsum("ij,bcyxjk,lk->bcyxil", m, _tiles(np.abs(x) if absolute else x), m)


def _wino_u(w, absolute=False):
    m = np.abs(G) if absolute else G
    return np.einsum("ij,ocjk,lk->ocil", m, np.abs(w) if absolute else w, m)


def _wino_out(M, H, W, absolute=False):
    """[B,O,ty,tx,4,4] products summed over the input channels -> [B,O,H,W]."""
    m = np.abs(AT) if absolute else AT
    Y = np.einsum("pi,boyxil,ql->boypxq", m, M, m)
    B, O, ty, _, tx, _ = Y.shape
    return Y.reshape(B, O, 2 * ty, 2 * tx)[:, :, :H, :W]


def _wino_conv(x, w):
    x, w = x.double().numpy(), w.double().numpy()
    M = np.einsum("bcyxil,ocil->boyxil", _wino_v(x), _wino_u(w))
    return _wino_out(M, x.shape[2], x.shape[3])


def test_numpy_winograd_is_the_convolution():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 5, 9, 11, generator=g), torch.randn(7, 5, 3, 3, generator=g)
    ref = F.conv2d(x.double(), w.double(), padding=1).numpy()
    assert np.abs(_wino_conv(x, w) - ref).max() <= 1e-13 * np.abs(ref).max()


# ---- the packers' power-of-two weight scale and the propagated bound

def _weight_scale(w, wino):
    """k_wino_pack_fp16 / k_pack_weight_h3: the largest power of two s with 2.25 max |w| s < 2^13 (Winograd) or max |w| s < 2^13."""
    wmax = np.float32(w.abs().max().item())
    _, e = np.frexp(np.float32(2.25) * wmax if wino else wmax)
    return 2.0 ** (13 - int(e))


def _dw(u, s):
    return h2_bound(np.abs(u) * s) / s


def _bound(form, shape, x, w, ref, pooled=False):
    """What the form's header allows, elementwise, in float64: the representation error of both operands' piece pairs (h2_bound;
    the weights after their power-of-two scale), the dropped product of the two second pieces (each below 2^-10 of its value by
    truncation), f32 roundings of the transforms, f32 accumulation as K 2^-24 sum |u| |v|, and one rounding of the output."""
    B, Cin, Hi, Wi, Cout, k, stride, pad = shape
    drop = 2.0 ** -20 if form.three else 0.0
    if form.kind == "wino":
        xn, wn = x.double().numpy(), w.double().numpy()
        V, U, Va, Ua = _wino_v(xn), _wino_u(wn), _wino_v(xn, True), _wino_u(wn, True)
        dV = h2_bound(np.abs(V)) + 3 * 2.0 ** -24 * Va                       # two levels of f32 additions in the input transform
        dU = _dw(U, _weight_scale(w, True)) + 6 * 2.0 ** -24 * Ua            # four in the packer's
        sum_c = lambda a, b: np.einsum("bcyxil,ocil->boyxil", a, b)
        prod = sum_c(np.abs(V), np.abs(U))
        M = sum_c(dV, np.abs(U)) + sum_c(np.abs(V) + dV, dU) + (drop + (Cin + 8) * 2.0 ** -24) * prod
        e = torch.from_numpy(_wino_out(M, Hi, Wi, True))
    else:
        conv = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad)
        ax, aw = x.double().abs(), w.double().abs()
        dx = torch.from_numpy(h2_bound(ax.numpy()))
        dw = torch.from_numpy(_dw(aw.numpy(), _weight_scale(w, False)))
        e = conv(dx, aw) + conv(ax + dx, dw) + (drop + (Cin * k * k + 8) * 2.0 ** -24) * conv(ax, aw)
    if pooled:
        e = F.max_pool2d(e, 3, 2, 1)                                           # |max a - max b| <= max |a - b|; ReLU shrinks differences
    return e + 2.0 ** -23 * ref.abs()


# ======================================================================================================================
# 1. exact operands

def _conv_int(xi, wi, stride, pad):
    """int64 convolution, tap by tap."""
    B, C, H, W = xi.shape
    O, _, k, _ = wi.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.pad(xi, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((B, O, Ho, Wo), np.int64)
    for i in range(k):
        for j in range(k):
            out += np.einsum("bchw,oc->bohw", xp[:, :, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride], wi[:, :, i, j])
    return out


def _abs_sum_bound(kind, shape, x, w):
    """The largest value any partial sum of any form can take: sum |x| |w| through the form's own transforms."""
    if kind == "wino":
        xn, wn = x.double().numpy(), w.double().numpy()
        M = np.einsum("bcyxil,ocil->boyxil", np.abs(_wino_v(xn)), np.abs(_wino_u(wn)))      # (V and U themselves are exact on these grids)
        return float(_wino_out(M, shape[2], shape[3], True).max())
    return float(F.conv2d(x.double().abs(), w.double().abs(), stride=shape[6], padding=shape[7]).max())


@functools.lru_cache(maxsize=None)
def _exact_case(shape, kind, tier):
    """Operands on a grid on which every intermediate of every form is exact, the float64 reference, and the proof of the premise.

    tier 0 — everything fits the FIRST piece of every form: x multiples of 2^-4 in [-2, 2], w multiples of 2^-4 in [-1, 1] (a
    third of them zero), bias a multiple of 2^-4, folded-BatchNorm scale a power of two.  A Winograd input value (a signed sum of
    four activations) and U = G g G^T (a multiple of 2^-6, |U| <= 2.25) have <= 8 significant bits; every product is exact in
    f32; every partial sum is a multiple of 2^-10 whose size the absolute-value sum bounds below 2^14.

    tier a (12, 15 or 16) — one operand of every product needs ALL pieces, the other one piece: in even input channels
    x = p + t 2^-a and w = q, in odd channels x = q and w = p + t 2^-a, with p, t, q in {-1, 0, 1} (for a > 12 a third
    digit u 2^-8 between the two, so that each of three bf16 pieces gets one).  A transformed wide value
    P + T 2^-a (|P|, |T| <= 4) spans <= a + 3 bits: 15 for a = 12 — two fp16 pieces, two bf16 pieces — and 18 / 19 for a = 15 / 16
    — three bf16 pieces.  Every product of pieces is exact, a multiple of 2^-(a + 2) (2^-a outside the Winograd forms), and so is
    every partial sum as long as sum |x| |w| through the form's transforms stays below 2^(22 - a) (2^(24 - a)): asserted.  The
    product of two SECOND pieces is never non-zero on this grid (no grid makes it so: two operands of more than 11 bits each multiply
    to more than 22 bits below the leading one, and an f32 sum of several such terms is not exact) — so the three-product forms
    must be exact on it as well."""
    B, Cin, Hi, Wi, Cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(1000 * tier + Cin + Cout + Hi)
    ri = lambda lo, hi, size: torch.randint(lo, hi + 1, size, generator=g)
    xs, ws = (B, Cin, Hi, Wi), (Cout, Cin, k, k)
    if tier == 0:
        unit = 16
        xi = ri(-32, 32, xs)
        wi = ri(-16, 16, ws) * (ri(0, 2, ws) > 0)
        shift = ri(-32, 32, (Cout,)).double() / 16
        scale = None if kind == "lateral" else 2.0 ** ri(-1, 1, (Cout,)).double()
    else:
        unit = 2 ** tier
        mid = 0 if tier == 12 else unit // 256                                # a third digit at 2^-8: one per bf16 piece
        wide = lambda size: ri(-1, 1, size) * unit + ri(-1, 1, size) * mid + ri(-1, 1, size)
        narrow = lambda size: ri(-1, 1, size) * unit
        even = (torch.arange(Cin) % 2 == 0)
        xi = torch.where(even.view(1, -1, 1, 1), wide(xs), narrow(xs))
        wi = torch.where(even.view(1, -1, 1, 1), narrow(ws), wide(ws))
        shift, scale = ri(-2, 2, (Cout,)).double(), None
    x, w = (xi.double() / unit).float(), (wi.double() / unit).float()
    assert torch.equal(x.double() * unit, xi.double()) and torch.equal(w.double() * unit, wi.double())
    conv = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    ci = _conv_int(xi.numpy(), wi.numpy(), stride, pad)
    assert np.array_equal(conv.numpy() * float(unit) ** 2, ci.astype(np.float64)), "float64 is not exact on this grid"
    form = Form("ref", 0, kind=kind)
    kw = dict(scale=None if scale is None else scale.float(), shift=shift.float(), relu=True)
    ref = _ref(form, shape, x, w, **kw)
    assert ref.abs().max().item() * 2.0 ** 10 < 2.0 ** 24
    grid = 2.0 ** 10 if tier == 0 else 2.0 ** (tier + 2) if kind == "wino" else 2.0 ** tier
    worst = _abs_sum_bound(kind, shape, x, w) * (2.0 if scale is not None else 1.0) + shift.abs().max().item()
    assert worst * grid < 2.0 ** 24, (worst, grid)
    assert torch.equal(ref.float().double(), ref)
    return x, w, kw, ref


def _assert_bitwise(out, ref, what):
    want = ref.float()
    if not torch.equal(out, want):
        bad = ~(out == want)
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from float64; the first at {idx}: "
                             f"got {out[idx].item()!r}, want {want[idx].item()!r}")


def _geometry_packs(shape):
    from fastposecnn_amd import _native as nat
    out = (ctypes.c_int64 * 8)()
    nat.check(nat.lib().fpc_wino_pack_geometry(shape[2], shape[3], shape[0], shape[1], 0, out), "geometry")
    return out[0] > 1


def _w(n):
    return Form(str(n), n, kind="wino", three=n in (-9, -10))


EXACT = [(F32, S3B), (F32, DIRECT), (F32, S3A),                              # fast loader, stride 2, the per-lane tap decode (Cin 16)
         (Form("f32-split3", 3, 64, 64), DIRECT), (Form("f32-two-launch", 103, 64, 64), DIRECT)]
EXACT += [(_w(n), s) for n in (-1, -2, -3, -4, -5, -7, -8) for s in (S3A, S3C)]
EXACT += [(_w(-6), S3A128), (_w(-6), S3C128), (W9, S3B), (W10, PACK1), (W10, PACK2)]
EXACT += [(BF3, S3B), (BF3, DIRECT), (Form("1002", 1002, 64, 64), DIRECT),
          (H3, S3B), (H3, DIRECT), (Form("6002", 6002, 64, 64, three=True), DIRECT), (Form("6102", 6102, 64, 64, three=True), DIRECT),
          (LAT_BF3, LATERAL), (Form("2001", 2001, kind="lateral"), LATERAL), (LAT_H3, LATERAL), (Form("7001", 7001, kind="lateral", three=True), LATERAL),
          (Form("4000", 4000, kind="pw"), POINTWISE), (Form("4001", 4001, kind="pw"), POINTWISE),
          (STEM_BF3, STEM_SHAPE), (STEM_H3, STEM_SHAPE)]
_case_id = lambda c: f"{c[0].name}-{c[1][1]}x{c[1][2]}x{c[1][3]}-{c[1][4]}" + (f"-2^-{c[2]}" if len(c) > 2 else "")


@pytest.mark.parametrize("case", EXACT, ids=_case_id)
def test_every_form_is_exact_on_single_piece_operands(lib, dev, case):
    """Tier 0 of _exact_case: every second and third piece is zero, every product and sum exact — torch.equal with float64."""
    form, shape = case
    if form.nsplit == -10:
        assert _geometry_packs(shape), "the case does not pack"
    kind = "wino" if shape[5] == 3 and shape[6] == 1 else form.kind      # the bound of the premise through the Winograd transforms too
    x, w, kw, ref = _exact_case(shape, kind, 0)
    out = _run(dev, form, shape, x, w, **kw)
    if form.nsplit == STEM_POOL:
        ref = F.max_pool2d(ref, 3, 2, 1)
    _assert_bitwise(out, ref, f"request {form.name} on {shape}")


# the forms that keep ALL piece products on a grid that needs them (a = 12: two pieces of either kind; a = 15 through the Winograd
# transforms and 16 elsewhere: three bf16 pieces), and the three-product forms, which lose nothing on it either.  Shapes: the
# largest of the tier-0 ones whose premise holds.
ALL_PIECES = [(W8, S3A, 12), (W8, S3C, 12), (W9, S3B, 12), (W10, PACK2, 12), (H3, S3B, 12), (H3, DIRECT, 12), (LAT_H3, LATERAL, 12),
              (STEM_H3, STEM_SHAPE, 12),
              (W7, S3A, 12), (_w(-5), S3A, 12), (_w(-6), S3A128, 12), (BF3, S3B, 12), (LAT_BF3, LATERAL, 12), (STEM_BF3, STEM_SHAPE, 12),
              (Form("4000", 4000, kind="pw"), POINTWISE, 12),
              (W7, S3TINY, 15), (_w(-5), S3TINY, 15), (BF3, S3B, 16), (LAT_BF3, LATERAL, 16), (STEM_BF3, STEM_SHAPE, 16),
              (Form("4001", 4001, kind="pw"), POINTWISE, 16)]


@pytest.mark.parametrize("case", ALL_PIECES, ids=_case_id)
def test_forms_are_exact_on_operands_that_need_every_piece(lib, dev, case):
    """Tiers 12, 15 and 16 of _exact_case.  A zeroed or mis-paired second (third) piece, or a dropped h2 g1 / h1 g2 product, changes
    bits 13 .. 15 (17 .. 19) of these outputs."""
    form, shape, tier = case
    x, w, kw, ref = _exact_case(shape, form.kind, tier)
    for v in ((_wino_v(x.double().numpy()), _wino_u(w.double().numpy())) if form.kind == "wino" else (x.numpy(), w.numpy())):
        last = split_h2(v.astype(np.float32))[1] if tier == 12 else split_bf3(v.astype(np.float32))[2]
        assert np.count_nonzero(last) > v.size // 100, "the grid does not reach the last piece"
    out = _run(dev, form, shape, x, w, **kw)
    if form.nsplit == STEM_POOL:
        ref = F.max_pool2d(ref, 3, 2, 1)
    _assert_bitwise(out, ref, f"request {form.name} on {shape}, grid 2^-{tier}")


# ======================================================================================================================
# 3. worst-case and channel-disparate operands, inside the envelope

PAIRS = [(W8, W7, S3B128, 4.0), (W9, W7, S3B128, 6.0), (W10, W7, PACK2_128, 6.0), (H3, BF3, DIRECT, 6.0), (LAT_H3, LAT_BF3, LATERAL, 6.0),
         (STEM_H3, STEM_BF3, STEM_SHAPE, 6.0)]
FULL = 2.0 - 2.0 ** -23                                                       # all 24 mantissa bits set


def _family(name, shape):
    B, Cin, Hi, Wi, Cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(len(name) * 131 + Cin + Cout)
    xs, ws = (B, Cin, Hi, Wi), (Cout, Cin, k, k)
    sign = lambda size: torch.randint(0, 2, size, generator=g).float() * 2 - 1
    if name.startswith("coherent"):
        # every truncation residual is the largest its binade allows; with x, w >= 0 (post-ReLU data against a smoothing kernel)
        # they all add
        x = FULL * 2.0 ** torch.randint(-2, 3, xs, generator=g).double()
        w = FULL * 2.0 ** torch.randint(-6, -2, ws, generator=g).double()
        if name == "coherent-signed":
            x, w = x * sign(xs), w * sign(ws)
        return x.float(), w.float()
    if name == "disparity":
        # a checkpoint with folded BatchNorm and dead channels: per-channel powers of two on both operands
        a = torch.randint(-8, 5, (Cin,), generator=g).double()
        b = torch.randint(-12, 1, (Cout,), generator=g).double()
        x = (torch.randn(xs, generator=g).double() + 0.5).relu() * (2.0 ** a).view(1, -1, 1, 1)
        w = (torch.randn(ws, generator=g).double() + 0.5) / (Cin * k * k) ** 0.5 * (2.0 ** b).view(-1, 1, 1, 1)
        return x.float(), w.float()
    raise KeyError(name)


def _edge_weights(shape, wmax):
    """|w| <= 0.9 wmax, except one whole filter tap set (output channel 0, input channel 0) at wmax: U[1][1] = 2.25 wmax there."""
    Cout, Cin, k = shape[4], shape[1], shape[5]
    g = torch.Generator().manual_seed(7)
    w = (torch.rand((Cout, Cin, k, k), generator=g) * 1.8 - 0.9) * float(wmax)
    w[0, 0] = float(wmax)
    return w.float()


def _hold_bars(dev, form, sib, shape, ratio, x, w, what):
    pooled = form.nsplit == STEM_POOL
    ref = _ref(form, shape, x, w, pooled=pooled)
    out = _run(dev, form, shape, x, w)
    ref_s = _run(dev, sib, shape, x, w, pool=pooled)
    assert torch.isfinite(out).all() and torch.isfinite(ref_s).all()
    bound = _bound(form, shape, x, w, ref, pooled=pooled)
    err, err_s = (out.double() - ref).abs(), (ref_s.double() - ref).abs()
    ce, cm = _chan_err(out, ref)
    ces, _ = _chan_err(ref_s, ref)
    scale = ref.abs().max().item()
    over = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: form {form.name} err {err.max().item():.3e} (worst channel {(ce / cm).max().item():.3e} of its own max), sibling "
          f"{sib.name} err {err_s.max().item():.3e} (worst channel {(ces / cm).max().item():.3e}), max |ref| {scale:.3e}, "
          f"err / bound {over:.3f}")
    assert (cm > 0).all()
    assert (ces <= 2e-5 * cm).all(), (what, "the sibling leaves the per-channel bar: the operands are out of range", (ces / cm).max().item())
    assert (ce <= 2e-5 * cm).all(), (what, "per-channel bar", (ce / cm).max().item(), int((ce / cm).argmax()))
    assert err.max().item() <= ratio * err_s.max().item() + 2.0 ** -23 * scale, (what, "against the sibling", err.max().item(), err_s.max().item())
    assert (err <= bound).all(), (what, "the propagated bound of the header's statement", over)


@pytest.mark.parametrize("family", ["coherent-signed", "coherent-positive", "disparity"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p[0].name)
def test_fp16_forms_on_worst_case_operands(lib, dev, pair, family):
    """(a) 2e-5 of every output channel's own maximum, (b) within 4x (all four products) / 6x (three) of the bf16 x 3 sibling plus
    one f32 rounding of the output, (c) inside the bound propagated from h2_bound.  Every figure is printed before it is asserted."""
    form, sib, shape, ratio = pair
    x, w = _family(family, shape)
    _hold_bars(dev, form, sib, shape, ratio, x, w, family)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p[0].name)
def test_fp16_forms_with_the_weight_maximum_on_a_binade_edge(lib, dev, pair):
    """max |w| = 2^-3 (the direct forms' rule changes its exponent there) and the f32 next to 2^-1 / 2.25 (where 2.25 max |w| crosses
    a power of two: the Winograd packer's rule), each with its predecessor and successor: max |U s| lands on both sides of 2^13.
    What this sees is a scale that disagrees with the 1 / s the kernel multiplies by, or weights that leave fp16 at the edge.  It cannot
    see a packer that moves BOTH by one binade: s and 1 / s come from the same exponent, max |U s| < 2^13 leaves three binades below
    65 504, and one binade more or less of the 2^-24 / s floor is far inside every bar here — such a shift is harmless."""
    form, sib, shape, ratio = pair
    g = torch.Generator().manual_seed(3)
    x = torch.randn((shape[0], shape[1], shape[2], shape[3]), generator=g)
    wino = form.kind == "wino"
    c = np.float32(2.25 if wino else 1.0)
    tops = []
    for centre in (np.float32(2.0 ** -3), np.float32(2.0 ** -1 / 2.25)):
        for wmax in (np.nextafter(centre, np.float32(0)), centre, np.nextafter(centre, np.float32(1))):
            w = _edge_weights(shape, wmax)
            assert w.abs().max().item() == float(wmax)
            tops.append(float(c * wmax) * _weight_scale(w, wino))              # the packer's own rule, restated
            assert 2.0 ** 12 <= tops[-1] < 2.0 ** 13
            _hold_bars(dev, form, sib, shape, ratio, x, w, f"max |w| = {float(wmax)!r}")
    assert min(tops) < 2.0 ** 12 * (1 + 2.0 ** -20) and max(tops) > 2.0 ** 13 * (1 - 2.0 ** -20), tops


# ======================================================================================================================
# 4. scale behaviour

H2_FORMS = [(W8, S3B128), (W9, S3B128), (W10, PACK2_128), (H3, DIRECT), (Form("6102", 6102, 64, 64, three=True), DIRECT), (LAT_H3, LATERAL),
            (STEM_H3, STEM_SHAPE)]
RANGE_FREE = [(F32, S3B), (_w(-1), S3C), (_w(-5), S3C), (_w(-6), S3C128), (W7, S3C), (BF3, S3B), (LAT_BF3, LATERAL),
              (Form("4000", 4000, kind="pw"), POINTWISE), (STEM_BF3, STEM_SHAPE)]
_form_id = lambda c: f"{c[0].name}"


@functools.lru_cache(maxsize=None)
def _normal_operands(shape):
    B, Cin, Hi, Wi, Cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(Cin + Cout + Hi + 17)
    return torch.randn((B, Cin, Hi, Wi), generator=g), torch.randn((Cout, Cin, k, k), generator=g) / (Cin * k * k) ** 0.5


@pytest.mark.parametrize("case", H2_FORMS, ids=_form_id)
def test_weight_scale_is_exactly_equivariant(lib, dev, case):
    """out(x, 2^e w) = 2^e out(x, w) bit for bit: the device scale moves by 2^-e and the packed image is the same.  The packers clamp
    the scale's exponent to +-100, i.e. max |w| within about 2^-87 .. 2^113: 2^+-24 around N(0, 1) / sqrt(fan-in) is far inside.
    All-zero weights give zeros; one NaN weight gives a non-finite output and no fault."""
    form, shape = case
    x, w = _normal_operands(shape)
    base = _run(dev, form, shape, x, w)
    assert torch.isfinite(base).all() and base.abs().max().item() > 0.1
    for e in (-24, -12, -1, 1, 12, 24):
        out = _run(dev, form, shape, x, w * 2.0 ** e)
        assert torch.equal(out, base * 2.0 ** e), (form.name, e, (out.double() - base.double() * 2.0 ** e).abs().max().item())
    zero = _run(dev, form, shape, x, torch.zeros_like(w))
    assert torch.equal(zero, torch.zeros_like(zero))
    wn = w.clone()
    wn[1, 2 % shape[1], 0, 0] = float("nan")
    out = _run(dev, form, shape, x, wn)
    # only output channel 1 reads the NaN: it is not finite (3100: its ReLU and max-pool may return the other operand of a NaN, so
    # nothing is stated about that channel there), and every other channel is the convolution still — on another weight scale (a NaN
    # maximum leaves the weights unscaled), hence to the 2e-5 bar and not bit for bit
    assert form.kind == "stem" or not torch.isfinite(out[:, 1]).all()
    others = [c for c in range(shape[4]) if c != 1]
    ref = _ref(form, shape, x, w, pooled=form.nsplit == STEM_POOL)[:, others]
    assert torch.isfinite(out[:, others]).all()
    assert (out[:, others].double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.parametrize("case", [c for c in H2_FORMS if c[0].nsplit != STEM_POOL], ids=_form_id)
def test_activations_below_the_envelope_lose_only_the_absolute_floor(lib, dev, case):
    """(Not 3100: through its max-pool an elementwise statement about the convolution's error does not carry over.)
    x 2^-e, e = 0 .. 16, on one operand set: |err(e)| <= 2^-e |err(0)| + floor elementwise, floor = fp16's subnormal spacing
    (h2_bound's absolute term) times sum |U| of the output channel, U the transformed weights (the weights themselves for the direct
    forms).  The 2e-5 bar of the tensor's own scale still holds for e <= 3."""
    form, shape = case
    x, w = _normal_operands(shape)
    wd = w.double()
    absu = np.abs(_wino_u(wd.numpy())).sum((1, 2, 3)) if form.kind == "wino" else wd.abs().sum((1, 2, 3)).numpy()
    floor = (H2_ABS * torch.from_numpy(np.asarray(absu))).view(1, -1, 1, 1)
    err0, last = None, -1
    for e in range(17):
        xs = x * 2.0 ** -e
        ref = _ref(form, shape, xs, w)
        err = (_run(dev, form, shape, xs, w).double() - ref).abs()
        rel = err.max().item() / ref.abs().max().item()
        if rel <= 2e-5 and last == e - 1:
            last = e
        print(f"form {form.name} activations x 2^-{e}: err {rel:.3e} of max |ref|")
        if e == 0:
            err0 = err
        assert (err <= 2.0 ** -e * err0 + floor).all(), (form.name, e, (err - 2.0 ** -e * err0 - floor).max().item())
        assert e > 3 or rel <= 2e-5, (form.name, e, rel)
    print(f"form {form.name}: 2e-5 of the tensor's scale held down to x 2^-{last}")


@pytest.mark.parametrize("case", H2_FORMS, ids=_form_id)
def test_activations_at_the_top_of_the_envelope(lib, dev, case):
    """(A departure from the issue on purpose: it asked for 2e-5 just under "the saturation point", which the headers gave as 131 008.
    The emulation shows that full precision ends at 2^16, so 2e-5 is asserted there and only the propagated bound above it.)
    4 max |x| (a transformed value is a signed sum of four activations) just under 2^16, where the first piece's range ends: the
    2e-5 bar holds.  Up to 131 008 = 2 x 65 504 the second piece carries the excess on 11 bits (h2_bound: up to 2^-12 of the
    value): the propagated bound holds.  One value beyond that saturates: finite, and the outputs it does not reach are unaffected."""
    form, shape = case
    pooled = form.nsplit == STEM_POOL
    x, w = _normal_operands(shape)
    for top, bar in ((H2_FULL, 2e-5), (H2_SAT, None)):
        xs = (x.double() * (top * (1 - 2.0 ** -10) / 4 / x.abs().max().item())).float()
        assert 4 * xs.abs().max().item() < top
        ref = _ref(form, shape, xs, w, pooled=pooled)
        out = _run(dev, form, shape, xs, w)
        err = (out.double() - ref).abs()
        rel = err.max().item() / ref.abs().max().item()
        print(f"form {form.name} with 4 max |x| just under {top:.0f}: err {rel:.3e} of max |ref|")
        assert (err <= _bound(form, shape, xs, w, ref, pooled=pooled)).all(), (form.name, top)
        assert bar is None or rel <= bar, (form.name, top, rel)
    xs = x.clone()
    xs[0, 1, 5, 7] = 1.0e6
    out = _run(dev, form, shape, xs, w)
    assert torch.isfinite(out).all()
    ref = _ref(form, shape, xs, w, pooled=pooled)
    touched = _ref(form, shape, (xs == 1.0e6).float(), torch.ones_like(w), pooled=pooled) > 0
    if form.kind == "wino":
        touched = F.max_pool2d(touched.double(), 5, 1, 2) > 0              # the 4 x 4 input tiles of the neighbouring output tiles
    far = ~touched
    assert far.any() and ((out.double() - ref).abs()[far]).max().item() <= 2e-5 * ref[far].abs().max().item()


@pytest.mark.parametrize("case", RANGE_FREE, ids=_form_id)
def test_bf16_and_f32_forms_have_no_range_limit(lib, dev, case):
    """The same operands at 2^-30, 1 and 2^30 meet 2e-5 of their own scale."""
    form, shape = case
    x, w = _normal_operands(shape)
    for s in (2.0 ** -30, 1.0, 2.0 ** 30):
        xs = x * s
        ref = _ref(form, shape, xs, w)
        out = _run(dev, form, shape, xs, w)
        assert torch.isfinite(out).all()
        rel = (out.double() - ref).abs().max().item() / ref.abs().max().item()
        assert rel <= 2e-5, (form.name, s, rel)


# ======================================================================================================================
# 5. the network on parameters that are not random-init

FP16_CODES = lambda c: c in (-8, -9, -10, 3100, 5000) or 6000 <= c < 6200 or 7000 <= c < 7100
NET_B, NET_H, NET_W = 2, 64, 96


def _encoder(model):
    for mod in model.modules():
        if all(hasattr(mod, a) for a in ("conv1", "bn1", "relu", "maxpool", "layer1", "layer4")):
            return mod
    raise AssertionError("no ResNet encoder in the model")


def _laterals(model):
    out = []
    for mod in model.modules():
        if all(hasattr(mod, a) for a in ("p5", "p4", "p3", "p2", "seg_blocks")):
            out += [mod.p5, mod.p4.skip_conv, mod.p3.skip_conv, mod.p2.skip_conv]
    assert out
    return out


MEAN_SHIFT = 0.5      # of std / sqrt(fan-in): coherent over the fan-in, it adds half of what the random part does


def _checkpoint_like(m, seed=5):
    """Conv weights with a non-zero mean (MEAN_SHIFT), folded BatchNorm scale gamma / sqrt(var) log-uniform in
    [2^-2, 2^1] per channel, shifts of both signs."""
    g = torch.Generator().manual_seed(seed)
    enc = _encoder(m)
    with torch.no_grad():
        for mod in enc.modules():
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.add_(MEAN_SHIFT * mod.weight.std() / (mod.weight[0].numel()) ** 0.5)
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                fold = 2.0 ** (torch.rand(n, generator=g) * 3 - 2)
                mod.weight.copy_(fold * (mod.running_var + mod.eps).sqrt())
                mod.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                mod.bias.copy_(torch.randn(n, generator=g) * 0.2)


def _scale_stage_outputs(m, x, targets=(11.4, 12.0, 12.5, 13.0)):
    """The last BatchNorm of layer1 .. layer4 scaled by a power of two each (front to back, on float64 forwards) towards maxima of
    c2 .. c5 of 2^targets.  (A stage's identity path carries its input on: after layer1 the factors are small.)"""
    enc = _encoder(m)
    for name, target in zip(("layer1", "layer2", "layer3", "layer4"), targets):
        with torch.no_grad():
            feats = copy.deepcopy(enc).double()(x.double())
            top = feats[2 + ("layer1", "layer2", "layer3", "layer4").index(name)].abs().max().item()
            f = 2.0 ** round(target - np.log2(top))
            last = getattr(enc, name)[-1].bn2
            last.weight.mul_(f)
            last.bias.mul_(f)


def _reference(m, hp, x):
    """float64 module path with the maxima of what every 3x3 / stride-1 convolution reads and of c2 .. c5."""
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp)
    ref_m.HPARAM.USE_NATIVE_ENGINE = False
    seen, hooks = {}, []
    for name, mod in ref_m.named_modules():
        if isinstance(mod, torch.nn.Conv2d) and mod.kernel_size == (3, 3) and mod.stride == (1, 1):
            hooks.append(mod.register_forward_pre_hook(lambda _m, inp, name=name: seen.__setitem__(name, inp[0].abs().max().item())))
    with torch.no_grad():
        ref = ref_m.pure_model_forward(x.double())
        feats = _encoder(ref_m)(x.double())
    for h in hooks:
        h.remove()
    return ref, seen, [f.abs().max().item() for f in feats[2:]]


def _engine(m, dev, level):
    """Split level 0: f32 products.  1: every Winograd site on the bf16 x 3 form -7.  3 (the default level): every site that has an
    fp16-piece form ON it — Winograd sites on -9, s2.0 with the p2 lateral folded in, the direct and lateral sites on three
    products — not just where the autotuner picks them.  (Not the stem: 64 x 96 is below the smallest frame k_stem_pool_h3 takes;
    request 3100 is held to the same operands at the kernel level above and in the network by tests/test_gpu_stem_pool.py.)"""
    from fastposecnn_amd.engine import NetEngine
    eng = NetEngine(m, NET_B, NET_H, NET_W, dev, autotune=False, split_precision=level)
    if level == 1:
        assert eng.force_winograd(7) > 0
    if level == 3:
        assert eng.force_winograd(9) > 0
        eng.force_fold(1)
        assert eng.force_direct_h3(1) > 0
        codes = [p[2] for p in eng.conv_plans()]
        assert sum(1 for c in codes if FP16_CODES(c)) >= 20, codes
    else:
        assert not any(FP16_CODES(p[2]) for p in eng.conv_plans())
    return eng


def _net_errors(eng, x, ref, dev):
    with torch.no_grad():
        logits, _ = eng.forward(x.to(dev))
    return {k: (logits[k].cpu().double() - ref[k]).abs().max().item() / max(1.0, ref[k].abs().max().item())
            for k in ("mask", "quaternion", "scales", "xy", "z")}


@functools.lru_cache(maxsize=None)
def _net_case(name):
    from fastposecnn_amd import synth
    import fastposecnn_amd.lib as L
    m, hp = _model(L, None, "resnet18")
    x = torch.stack([synth.make_image(i, NET_H, NET_W) for i in range(NET_B)])
    if name == "checkpoint-like":
        _checkpoint_like(m)
    if name == "large":
        _scale_stage_outputs(m, x)
    if name == "tiny-pyramid":
        with torch.no_grad():
            for conv in _laterals(m):
                conv.weight.mul_(2.0 ** -10)
                conv.bias.mul_(2.0 ** -10)
    ref, seen, cmax = _reference(m, hp, x)
    return m, x, ref, seen, cmax


def _assert_scenario(name, m, seen, cmax):
    """Each parameter set is what it claims, on the float64 activations."""
    decoder = {k: v for k, v in seen.items() if "seg_blocks" in k and k.endswith("0.block.0")}      # the 3x3 sites that read p5 .. p2
    assert len(decoder) >= 4, sorted(seen)
    if name == "checkpoint-like":
        enc = _encoder(m)
        folds = torch.cat([(b.weight / (b.running_var + b.eps).sqrt()).detach() for b in enc.modules() if isinstance(b, torch.nn.BatchNorm2d)])
        assert folds.min().item() >= 0.25 and folds.max().item() <= 2.0 and folds.max().item() / folds.min().item() > 6
        assert all(c.weight.mean().item() > 0.5 * MEAN_SHIFT * c.weight.std().item() / c.weight[0].numel() ** 0.5 for c in enc.modules() if isinstance(c, torch.nn.Conv2d))
    if name in ("checkpoint-like", "large"):
        assert all(0 < 4 * v < H2_FULL for v in seen.values()), {k: v for k, v in seen.items() if not 4 * v < H2_FULL}
    if name == "large":
        assert all(2.0 ** 11 <= c <= 2.0 ** 14 for c in cmax), cmax
    if name == "tiny-pyramid":
        assert all(2.0 ** -8 < v < 2.0 ** -5 for v in decoder.values()), decoder      # every value far below the 2^-2 of the relative regime


@pytest.mark.parametrize("level", [0, 1, 3])
@pytest.mark.parametrize("name", ["checkpoint-like", "large"])
def test_network_on_checkpoint_like_and_large_parameters(lib, dev, name, level):
    """ResNet18-FPN, B = 2, 64 x 96, against the float64 module path at 1e-4 of each logit tensor's scale, at split levels 0, 1 and
    the default (3) with every fp16-piece site forced on (see _engine)."""
    m, x, ref, seen, cmax = _net_case(name)
    _assert_scenario(name, m, seen, cmax)
    eng = _engine(copy.deepcopy(m).to(dev), dev, level)
    errs = _net_errors(eng, x, ref, dev)
    print(name, "level", level, errs)
    assert max(errs.values()) <= 1e-4, (name, level, errs)


@pytest.mark.parametrize("level", [0, 1, 3])
def test_network_with_a_tiny_pyramid_below_the_envelope(lib, dev, level):
    """Every FPN lateral x 2^-10 (exact): the decoder's 3x3 sites read tensors of scale 2^-10, below the fp16 pieces' envelope.  The
    range-free levels meet the bar.  The default level (3, every fp16-piece site forced on) is the documented limit, not a bug: its
    error is printed and only held to be finite."""
    m, x, ref, seen, cmax = _net_case("tiny-pyramid")
    _assert_scenario("tiny-pyramid", m, seen, cmax)
    eng = _engine(copy.deepcopy(m).to(dev), dev, level)
    errs = _net_errors(eng, x, ref, dev)
    print("tiny-pyramid level", level, errs)
    assert all(np.isfinite(v) for v in errs.values())
    assert level == 3 or max(errs.values()) <= 1e-4, (level, errs)


@pytest.mark.parametrize("encoder", ["resnet18", "resnet50"])
def test_no_fp16_piece_form_without_split_f16(lib, dev, encoder):
    """HPARAM.ENGINE_SPLIT_F16 = False keeps EVERY fp16-piece form out of the autotuned plans: -8, -9, -10, 3100, 5000,
    6000 .. 6199 and 7000 .. 7099."""
    from fastposecnn_amd import synth
    m, hp = _model(lib, dev, encoder)
    hp.ENGINE_SPLIT_F16 = False
    m = m.to(dev)
    with torch.no_grad():
        m(torch.stack([synth.make_image(i, NET_H, NET_W) for i in range(NET_B)]).to(dev))
    assert m._engines
    codes = [p[2] for p in next(iter(m._engines.values())).conv_plans()]
    assert not any(FP16_CODES(c) for c in codes), codes
    # the control, independent of what the autotuner happens to time fastest: at this frame sites ARE eligible for an fp16-piece form
    # — with the flag off the request for one is refused (the fp16 images are not even packed); the next test is the other half
    eng = next(iter(m._engines.values()))
    with pytest.raises(RuntimeError):
        eng.force_direct_h3(1)
    assert not any(FP16_CODES(p[2]) for p in eng.conv_plans())


def test_fp16_piece_forms_are_eligible_at_the_frame_of_the_flag_test(lib, dev):
    """... and with the flag on (the default) the same request at the same frame puts ResNet18's direct sites on three fp16 piece
    products: the test above is about the flag, not about a frame at which no site could take those forms."""
    from fastposecnn_amd import synth
    m2, _ = _model(lib, dev, "resnet18")
    m2 = m2.to(dev)
    with torch.no_grad():
        m2(torch.stack([synth.make_image(i, NET_H, NET_W) for i in range(NET_B)]).to(dev))
    eng2 = next(iter(m2._engines.values()))
    eng2.force_direct_h3(1)
    assert any(6000 <= p[2] < 6200 or 7000 <= p[2] < 7100 for p in eng2.conv_plans()), eng2.conv_plans()
