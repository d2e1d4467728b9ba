"""The algebra behind s2.0's FPN p2 fold (csrc/wino_h3.hip, FOLD), in numpy float64:
    conv3x3(W, L c2 + b + up2_nearest(p3)) = conv3x3(W L, c2) + conv3x3(W, up2(p3)) + conv3x3(W, b 1_inside)
with the p3 term's Winograd F(2x2, 3x3) input transform zero in row 2 and column 2, and the bias term a table by border class."""
import numpy as np
import pytest

# the kernel's B^T rows (wino_tile.hpp, wino_frag: 0: d0-d2  1: d1+d2  2: d2-d1  3: d1-d3), G and A^T of F(2x2, 3x3) (k_wino_pack_fp16, the epilogue)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def conv3x3(x, w):
    """x [C, H, W], w [O, C, 3, 3], zero padding 1."""
    C, H, W = x.shape
    xp = np.zeros((C, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,chw->ohw", w[:, :, ky, kx], xp[:, ky:ky + H, kx:kx + W])
    return out


def up2(x):
    return x.repeat(2, axis=1).repeat(2, axis=2)


def bias_table(w, b):
    """k_fold_compose's table: [row class][column class][O], bit 0 = first row / column, bit 1 = last."""
    t = np.zeros((4, 4, w.shape[0]))
    for rc in range(4):
        for cc in range(4):
            for ky in range(rc & 1, 3 - ((rc >> 1) & 1)):
                for kx in range(cc & 1, 3 - ((cc >> 1) & 1)):
                    t[rc, cc] += w[:, :, ky, kx] @ b
    return t


def winograd_p3_term(w, p3, H, W):
    """conv3x3(W, up2(p3)) on F(2x2, 3x3) tiles whose input comes straight from the 3 x 3 low-resolution neighbourhood, transformed
    positions of row 2 / column 2 skipped (the kernel never issues them)."""
    O, C = w.shape[:2]
    U = np.einsum("ij,ocjk,lk->ocil", G, w, G)                       # [O, C, 4, 4]
    up = np.zeros((C, H + 4, W + 4))
    up[:, 1:H + 1, 1:W + 1] = up2(p3)
    out = np.zeros((O, H + 1, W + 1))
    for ty in range(0, H, 2):
        for tx in range(0, W, 2):
            d = up[:, ty:ty + 4, tx:tx + 4]
            V = np.einsum("ij,cjk,lk->cil", BT, d, BT)
            M = np.einsum("ocil,cil->oil", U, V)
            M[:, 2, :] = 0.0
            M[:, :, 2] = 0.0
            out[:, ty:ty + 2, tx:tx + 2] = np.einsum("ij,ojk,lk->oil", AT, M, AT)
    return out[:, :H, :W]


def test_upsampled_tile_transform_has_exact_zero_row_and_column_2():
    rng = np.random.default_rng(0)
    for _ in range(100):
        lo = rng.standard_normal((3, 3)).astype(np.float32)
        # a tile at even output coordinates: input rows / columns 2i-1 .. 2i+2 of the upsample = low-res [a, b, b, c]
        d = lo[[0, 1, 1, 2]][:, [0, 1, 1, 2]]
        e = BT.astype(np.float32) @ d                                   # float32, the kernel's own precision
        V = e @ BT.T.astype(np.float32)
        assert np.all(V[2, :] == 0.0) and np.all(V[:, 2] == 0.0)
        a, b, c = lo[0], lo[1], lo[2]
        assert np.array_equal(e[[0, 1, 3]], np.stack([a - b, 2 * b, b - c])[:, [0, 1, 1, 2]])


def test_kernel_transform_is_the_standard_one():
    """B^T d B, U = G g G^T and A^T M A are F(2x2, 3x3): they reproduce the direct correlation of a 4 x 4 tile exactly."""
    rng = np.random.default_rng(1)
    d, g = rng.standard_normal((4, 4)), rng.standard_normal((3, 3))
    M = (G @ g @ G.T) * (BT @ d @ BT.T)
    y = AT @ M @ AT.T
    ref = np.array([[np.sum(d[i:i + 3, j:j + 3] * g) for j in range(2)] for i in range(2)])
    assert np.allclose(y, ref, atol=1e-12, rtol=0)


@pytest.mark.parametrize("h3,w3", [(3, 4), (5, 3), (1, 1), (1, 6), (4, 1)])
def test_fold_reproduces_the_p2_convolution(h3, w3):
    """composed weights on c2 + the 9-term Winograd p3 branch + the border-class bias table = conv3x3(W, L c2 + b + up2(p3)) to
    1e-12; odd tile counts per patch, 2-pixel-wide maps (1 low-res pixel) and every border class."""
    rng = np.random.default_rng(h3 * 10 + w3)
    O, Cm, Ck = 8, 12, 5
    H, W = 2 * h3, 2 * w3
    c2 = rng.standard_normal((Ck, H, W))
    p3 = rng.standard_normal((Cm, h3, w3))
    L = rng.standard_normal((Cm, Ck))
    b = rng.standard_normal(Cm)
    w = rng.standard_normal((O, Cm, 3, 3))
    ref = conv3x3(np.einsum("ck,khw->chw", L, c2) + b[:, None, None] + up2(p3), w)
    wc = np.einsum("ocyx,ck->okyx", w, L)
    t = bias_table(w, b)
    rc = (np.arange(H) == 0).astype(int) | ((np.arange(H) == H - 1).astype(int) << 1)
    cc = (np.arange(W) == 0).astype(int) | ((np.arange(W) == W - 1).astype(int) << 1)
    bias = t[rc[:, None], cc[None, :]].transpose(2, 0, 1)
    got = conv3x3(c2, wc) + winograd_p3_term(w, p3, H, W) + bias
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
