"""What tests/test_gpu_mbconv_train.py holds the EfficientNet depthwise gradient kernels to (csrc/depthwise.hip): the
cases, the operands and the kernels' formulas written out in float64 — the flipped stride-1 form and the per-parity stride-2 form of
the data gradient, the k k sums of the weight gradient — which tests/test_mbconv_train_host.py shows to BE float64 autograd through
F.conv2d(F.pad(x, static pads), w, groups = C).  Also include/fpc.h's slice count of the weight gradient, restated."""
import torch
import torch.nn.functional as F

KS = [(3, 1), (3, 2), (5, 1), (5, 2)]                                          # (k, stride)
# (B, Hi, Wi, C): a map on which every tap pads somewhere; strip and block tails; a mid-sized one; more than 256 channel quads
SHAPES = [(2, 2, 2, 4), (1, 6, 10, 32), (3, 30, 40, 144), (1, 16, 4, 1152)]
# for the weight gradient alone: several slices (asserted > 1 from the restated formula); fewer units than pixel slots
WGRAD_EXTRA = [(2, 22, 80, 8), (1, 4, 6, 8)]
SHAPES_ALL = SHAPES + WGRAD_EXTRA


def ids(cases):
    return ["B%d-%dx%d-C%d" % c for c in cases]


def pads(k, stride):
    """(before, after) per axis: efficientnet_pytorch's static "same" pad for an even extent"""
    return ((k - 1) // 2, (k - 1) // 2) if stride == 1 else ((k - 3) // 2, (k - 3) // 2 + 1)


def wgrad_slices(B, Ho, Wo, C, k):
    """include/fpc.h, fpc_mbconv_dw_wgrad: slice i takes rows [i B Ho / slices, (i + 1) B Ho / slices) of the (frame, row) list"""
    rows, nseg, chunks, slots = B * Ho, (Wo + 7) // 8, (C + 31) // 32, 32 if k == 3 else 8
    return max(1, min(max(1, 1024 // chunks), rows * nseg // slots, rows))


def operands(shape, k, stride, integer=False):
    """x, w, dy (NCHW, f32); integer: whole numbers in [-4, 4] (every product and sum exact in f32)"""
    B, Hi, Wi, C = shape
    g = torch.Generator().manual_seed(900 + 40 * SHAPES_ALL.index(shape) + 4 * k + 2 * stride + int(integer))
    if integer:
        draw = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    else:
        draw = lambda *s: torch.randn(s, generator=g)
    return draw(B, C, Hi, Wi), draw(C, 1, k, k), draw(B, C, Hi // stride, Wi // stride)


def autograd_ref(x, w, dy, k, stride):
    """(y, dx, dw) of F.conv2d(F.pad(x, static pads), w, groups = C) in float64 under autograd"""
    pb, pa = pads(k, stride)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(F.pad(xr, (pb, pa, pb, pa)), wr, None, stride, 0, 1, x.shape[1])
    dx, dw = torch.autograd.grad(y, [xr, wr], dy.double())
    return y.detach(), dx, dw


def dgrad_ref(dy, w, Hi, Wi, k, stride):
    """The kernels' data gradient in float64: dx[h][w] = sum dy[(h + pb - kh) / s][(w + pb - kw) / s] w[kh][kw] where the divisions
    are exact and the index is inside dy.  Stride 1: the flipped taps over a padded dy.  Stride 2: per output parity p the taps with
    p + pb - k even, from dy at offset (p + pb - k) / 2 — k = 3: dx[2a] = dy[a] w[0] + dy[a - 1] w[2], dx[2a + 1] = dy[a] w[1];
    k = 5: dx[2a] = dy[a] w[1] + dy[a - 1] w[3], dx[2a + 1] = dy[a + 1] w[0] + dy[a] w[2] + dy[a - 1] w[4]."""
    dy, w = dy.double(), w.double()
    B, C, Ho, Wo = dy.shape
    pb = pads(k, stride)[0]
    wc = w.view(1, C, k, k)
    dx = torch.zeros((B, C, Hi, Wi), dtype=torch.float64)
    if stride == 1:
        p = F.pad(dy, (pb, pb, pb, pb))
        for kh in range(k):
            for kw in range(k):
                dx += p[:, :, k - 1 - kh:k - 1 - kh + Hi, k - 1 - kw:k - 1 - kw + Wi] * wc[:, :, kh:kh + 1, kw:kw + 1]
        return dx
    taps = {p: [(t, (p + pb - t) // 2) for t in range(k) if (p + pb - t) % 2 == 0] for p in (0, 1)}
    assert taps == ({0: [(0, 0), (2, -1)], 1: [(1, 0)]} if k == 3 else {0: [(1, 0), (3, -1)], 1: [(0, 1), (2, 0), (4, -1)]})
    p = F.pad(dy, (1, 1, 1, 1))                          # dy[a - 1], dy[a + 1] outside the map: zero
    for py in range(2):
        for px in range(2):
            acc = torch.zeros((B, C, Ho, Wo), dtype=torch.float64)
            for ky, oy in taps[py]:
                for kx, ox in taps[px]:
                    acc += p[:, :, 1 + oy:1 + oy + Ho, 1 + ox:1 + ox + Wo] * wc[:, :, ky:ky + 1, kx:kx + 1]
            dx[:, :, py::2, px::2] = acc
    return dx


def wgrad_ref(x, dy, k, stride):
    """dw[c][kh][kw] = sum over b, ho, wo of dy[b, c, ho, wo] x[b, c, s ho + kh - pb, s wo + kw - pb] (zero outside x), float64"""
    x, dy = x.double(), dy.double()
    B, C, Ho, Wo = dy.shape
    pb = pads(k, stride)[0]
    p = F.pad(x, (pb, k, pb, k))                         # (more than enough after: the windows below stay inside)
    dw = torch.zeros((C, 1, k, k), dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            win = p[:, :, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            dw[:, 0, kh, kw] = (win * dy).sum((0, 2, 3))
    return dw
