"""References of the native stem / max-pool training path (tests/test_stem_train_host.py, tests/test_gpu_stem_train.py): float64
torch on the CPU, and a pure-numpy restatement of the gather rule k_maxpool3x3s2_bwd implements."""
import numpy as np
import torch
import torch.nn.functional as F


def close(a, ref, tol):
    """|a - ref|max <= tol max(1, |ref|max), the project's bar; returns (ok, error, bound)."""
    err = (a.detach().double().cpu() - ref.double()).abs().max().item()
    bound = tol * max(1.0, ref.abs().max().item())
    return err <= bound, err, bound


def stem_forward_ref(img, w):
    """float64 conv2d(img [B,3,H,W], w [64,3,7,7], stride 2, pad 3) on the CPU."""
    return F.conv2d(img.double().cpu(), w.double().cpu(), None, 2, 3)


def stem_wgrad_ref(img, dy):
    """float64 weight gradient of the stem: img [B,3,H,W], dy [B,64,H/2,W/2] (NCHW) -> [64,3,7,7]."""
    w = torch.zeros((64, 3, 7, 7), dtype=torch.float64, requires_grad=True)
    F.conv2d(img.double().cpu(), w, None, 2, 3).backward(dy.double().cpu())
    return w.grad.detach()


def maxpool_ref(x, dy=None):
    """F.max_pool2d(x, 3, 2, 1) in x's dtype on the CPU and, with dy, its autograd input gradient."""
    xr = x.detach().cpu().clone().requires_grad_(dy is not None)
    y = F.max_pool2d(xr, 3, 2, 1)
    if dy is None:
        return y.detach()
    y.backward(dy.detach().cpu().to(xr.dtype))
    return y.detach(), xr.grad.detach()


def maxpool_bwd_gather(x, dy):
    """The gather rule, element by element of dx, in numpy (x [B,C,H,W], dy [B,C,Ho,Wo]; any float dtype): an element lies in the
    windows o = i // 2 and, for odd i, (i + 1) // 2 where that window exists; it takes a window's dy where every in-bounds
    element scanned before it (row-major) is smaller and none scanned after it is larger — torch's first-maximum rule; the
    contributions are added in (window row, window column) order."""
    x, dy = np.asarray(x), np.asarray(dy)
    B, C, H, W = x.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    assert (Ho, Wo) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    dx = np.full(x.shape, np.nan, dtype=x.dtype)
    for iy in range(H):
        for ix in range(W):
            v = x[:, :, iy, ix]
            total = np.zeros((B, C), dtype=x.dtype)
            for oy in range(iy // 2, min((iy + 1) // 2, Ho - 1) + 1):
                for ox in range(ix // 2, min((ix + 1) // 2, Wo - 1) + 1):
                    win = np.ones((B, C), dtype=bool)
                    for hy in range(2 * oy - 1, 2 * oy + 2):
                        for wx in range(2 * ox - 1, 2 * ox + 2):
                            if hy < 0 or hy >= H or wx < 0 or wx >= W or (hy == iy and wx == ix):
                                continue
                            e = x[:, :, hy, wx]
                            win &= (e < v) if (hy, wx) < (iy, ix) else (e <= v)
                    total = total + np.where(win, dy[:, :, oy, ox], 0).astype(x.dtype)
            dx[:, :, iy, ix] = total
    return dx


def tie_heavy(shape, seed, dtype=torch.float32):
    """relu(randn) — half of it exact zeros — with channel 0 one constant plane."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(shape, generator=g)).to(dtype)
    x[:, 0] = 0.75
    return x
