"""What tests/test_gpu_dwconv_train.py holds the depthwise training kernels to (csrc/depthwise.hip): the cases, the operands and
the kernels' formulas written out in float64 — the stride-1 flipped form and the stride-2 parity form of the data gradient, the
nine sums of the weight gradient — which tests/test_dwconv_train_host.py shows to BE float64 autograd through
F.conv2d(groups = C).  Also include/fpc.h's slice count of the weight gradient, so that a test can say where the seams fall."""
import torch
import torch.nn.functional as F

# (B, Hi, Wi, C, stride).  The forward's DW_CASES (tests/test_gpu_mobilenet_v2.py) ...
DW_CASES = [(1, 1, 1, 32, 1), (3, 5, 7, 96, 1), (3, 5, 7, 96, 2), (2, 6, 8, 144, 2), (1, 2, 3, 960, 1), (2, 17, 33, 16, 1), (1, 9, 64, 4, 2)]
# ... and the stride-2 corners the parity form can get wrong: a 1 x 1 map (one block, three of its four pixels outside), one whole
# block, odd width / even height and the reverse (the last block column / row half outside, dy[a + 1] past the map)
S2_CORNERS = [(1, 1, 1, 32, 2), (1, 2, 2, 8, 2), (2, 6, 7, 4, 2), (1, 7, 6, 4, 2)]
CASES = DW_CASES + S2_CORNERS
# For the weight gradient, from the slice formula below: 22 rows in 3 slices (seams at rows 7 and 14, inside frame 0 and frame 1,
# 22 % 3 != 0) at stride 2 with odd sizes; and 3 rows of one segment: one slice of 3 units, fewer than a workgroup's 32 pixel slots
WGRAD_EXTRA = [(2, 21, 79, 8, 2), (1, 3, 5, 8, 1)]


def ids(cases):
    return [f"B{b}-{h}x{w}-C{c}-s{s}" for b, h, w, c, s in cases]


def out_hw(Hi, Wi, stride):
    return (Hi - 1) // stride + 1, (Wi - 1) // stride + 1


def wgrad_slices(B, Ho, Wo, C):
    """include/fpc.h, fpc_dwconv3x3_wgrad: slice i takes rows [i B Ho / slices, (i + 1) B Ho / slices) of the (frame, row) list"""
    rows, nseg, chunks = B * Ho, (Wo + 7) // 8, (C + 31) // 32
    return max(1, min(max(1, 1024 // chunks), rows * nseg // 32, rows))


def operands(case, integer=False):
    """x, w, dy (NCHW, f32) of a case; integer: whole numbers in [-4, 4] (every product and sum exact in f32)"""
    B, Hi, Wi, C, s = case
    Ho, Wo = out_hw(Hi, Wi, s)
    g = torch.Generator().manual_seed(500 + 10 * CASES_ALL.index(case) + int(integer))
    if integer:
        draw = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()
    else:
        draw = lambda *shape: torch.randn(shape, generator=g)
    return draw(B, C, Hi, Wi), draw(C, 1, 3, 3), draw(B, C, Ho, Wo)


CASES_ALL = CASES + WGRAD_EXTRA


def autograd_ref(x, w, dy, stride):
    """(y, dx, dw) of F.conv2d(groups = C) in float64 under autograd"""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride, 1, 1, x.shape[1])
    dx, dw = torch.autograd.grad(y, [xr, wr], dy.double())
    return y.detach(), dx, dw


def dgrad_ref(dy, w, Hi, Wi, stride):
    """The kernels' data gradient in float64.  Stride 1: dx[h][w] = sum dy[h + 1 - kh][w + 1 - kw] w[kh][kw].  Stride 2, per axis
    dx[2a] = dy[a] w[1], dx[2a + 1] = dy[a] w[2] + dy[a + 1] w[0]: the 2 x 2 block at (2a, 2b) from dy[a..a+1][b..b+1] (zero past
    Ho / Wo), nine products; rows and columns past Hi / Wi dropped."""
    dy, w = dy.double(), w.double()
    B, C, Ho, Wo = dy.shape
    wc = w.view(1, C, 3, 3)
    if stride == 1:
        p = F.pad(dy, (1, 1, 1, 1))
        dx = torch.zeros((B, C, Hi, Wi), dtype=torch.float64)
        for kh in range(3):
            for kw in range(3):
                dx += p[:, :, 2 - kh:2 - kh + Hi, 2 - kw:2 - kw + Wi] * wc[:, :, kh:kh + 1, kw:kw + 1]
        return dx
    p = F.pad(dy, (0, 1, 0, 1))                         # dy[a + 1], dy[b + 1] past the map: zero
    full = torch.zeros((B, C, 2 * Ho, 2 * Wo), dtype=torch.float64)
    taps = {0: ((1, 0),), 1: ((2, 0), (0, 1))}           # parity -> (tap index, offset into dy)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros((B, C, Ho, Wo), dtype=torch.float64)
            for ky, ry in taps[py]:
                for kx, rx in taps[px]:
                    acc += p[:, :, ry:ry + Ho, rx:rx + Wo] * wc[:, :, ky:ky + 1, kx:kx + 1]
            full[:, :, py::2, px::2] = acc
    return full[:, :, :Hi, :Wi].contiguous()


def wgrad_ref(x, dy, stride):
    """dw[c][kh][kw] = sum over b, ho, wo of dy[b, c, ho, wo] x[b, c, s ho + kh - 1, s wo + kw - 1] (zero outside x), float64"""
    x, dy = x.double(), dy.double()
    B, C, Ho, Wo = dy.shape
    p = F.pad(x, (1, 1, 1, 1))
    dw = torch.zeros((C, 1, 3, 3), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            win = p[:, :, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            dw[:, 0, kh, kw] = (win * dy).sum((0, 2, 3))
    return dw


def relu6_operands(index, shape):
    """BatchNorm + ReLU6 operands (x, gy NCHW; gamma, beta): pre-activations of spread ~4 about 3, more than a fifth on each clamp"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(700 + index)
    x = 2.0 * torch.randn(shape, generator=g) + 0.5
    gamma = 4.0 * (torch.rand(C, generator=g) + 0.5)
    beta = 3.0 + torch.randn(C, generator=g)
    gy = torch.randn(shape, generator=g)
    return x, gy, gamma, beta


RELU6_SHAPES = [(1, 32, 3, 5), (2, 96, 15, 20), (3, 144, 9, 7), (2, 960, 2, 3), (2, 16, 33, 17)]
