"""Shared by test_se_train_host.py and test_gpu_se_train.py: the six shapes, operands on which no ReLU sits on its kink, and the
float64 reference of the squeeze-and-excitation block's forward and backward written out as formulas (the host test pins it to
torch.autograd through SEModule + add + ReLU in float64).  Everything here runs on the CPU and is computed once per shape."""
import torch

# test_gpu_se.py's six (B, H, W, C, R): one pixel (dm / HW is the whole pool term); odd sizes and B = 3 (the batch-order sums);
# C / 4 > 256; several slabs with a ragged last one; two thread rows; Cr = 2 (the non-vector paths)
SHAPES = [(1, 1, 1, 64, 16), (3, 5, 7, 256, 16), (2, 15, 20, 2048, 16), (1, 37, 41, 128, 8), (2, 9, 64, 512, 16), (2, 3, 3, 64, 32)]
IDS = [f"B{b}-{h}x{w}-C{c}-R{r}" for b, h, w, c, r in SHAPES]

_CACHE = {}


def _away_from_zero(shape, g):
    """Values with |t| in [0.25, 1.25) and a random sign, float64."""
    mag = 0.25 + torch.rand(shape, generator=g, dtype=torch.float64)
    return torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)


def forward_ref(x, res, w1, b1, w2, b2):
    """float64: (mean, hidden pre-activation, gate, output pre-activation) from NHWC x / res and fc1 / fc2 as matrices."""
    x, res, w1, b1, w2, b2 = (t.double() for t in (x, res, w1, b1, w2, b2))
    m = x.mean(dim=(1, 2))
    a = m @ w1.t() + b1
    g = torch.sigmoid(a.relu() @ w2.t() + b2)
    z = x * g[:, None, None, :] + res
    return m, a, g, z


def backward_ref(x, res, w1, b1, w2, b2, gy):
    """float64, the formulas of the kernels: d = gy (y > 0); dg = sum_hw d x; dv = dg g (1 - g); dh = (h > 0) dv w2; dm = dh w1;
    dx = d g + dm / (H W); dres = d; dw2 = dv^T h; db2 = sum_b dv; dw1 = dh^T m; db1 = sum_b dh."""
    m, a, g, z = forward_ref(x, res, w1, b1, w2, b2)
    xd, gyd, w1d, w2d = x.double(), gy.double(), w1.double(), w2.double()
    B, H, W, C = x.shape
    h = a.relu()
    d = gyd * (z > 0)
    dg = (d * xd).sum(dim=(1, 2))
    dv = dg * g * (1 - g)
    dh = (a > 0) * (dv @ w2d)
    dm = dh @ w1d
    return {"y": z.relu(), "mean": m, "hidden": h, "gate": g, "pre_out": z, "pre_hidden": a,
            "dx": d * g[:, None, None, :] + dm[:, None, None, :] / (H * W), "dres": d,
            "dw2": dv.t() @ h, "db2": dv.sum(0), "dw1": dh.t() @ m, "db1": dh.sum(0)}


def operands(case):
    """f32 operands of `case` (x, res, gy NHWC; w1 [Cr][C], b1, w2 [C][Cr], b2) and their float64 reference.  x = randn + 1,
    w1 ~ randn / sqrt(C), w2 ~ randn / sqrt(Cr), b2 ~ randn; b1 puts frame 0's hidden pre-activations at +-[0.25, 1.25);
    res = t - x g_ref with |t| in [0.25, 1.25): every output pre-activation is t up to f32 rounding."""
    if case not in _CACHE:
        B, H, W, C, R = case
        Cr = C // R
        g = torch.Generator().manual_seed(7 + SHAPES.index(case))
        x = torch.randn((B, H, W, C), generator=g) + 1.0
        w1 = torch.randn((Cr, C), generator=g) / C ** 0.5
        w2 = torch.randn((C, Cr), generator=g) / Cr ** 0.5
        b2 = torch.randn(C, generator=g)
        b1 = (_away_from_zero((Cr,), g) - x[0].double().mean(dim=(0, 1)) @ w1.double().t()).float()
        gy = torch.randn((B, H, W, C), generator=g)
        _, _, g_ref, _ = forward_ref(x, torch.zeros_like(x), w1, b1, w2, b2)
        res = (_away_from_zero((B, H, W, C), g) - x.double() * g_ref[:, None, None, :]).float()
        ops = dict(x=x, res=res, w1=w1, b1=b1, w2=w2, b2=b2, gy=gy)
        _CACHE[case] = (ops, backward_ref(**ops))
    return _CACHE[case]
