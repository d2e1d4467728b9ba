"""References of the native VGG training path (tests/test_vgg_train_host.py, tests/test_gpu_vgg_train.py): float64 torch on the CPU —
F.conv2d under torch.autograd.grad for features.0's weight and bias gradient, F.max_pool2d under autograd for the 2x2 pool's input
gradient — and the inputs the pool tests share."""
import torch
import torch.nn.functional as F


def close(a, ref, tol):
    """|a - ref|max <= tol max(1, |ref|max), the project's bar; returns (ok, error, bound)."""
    err = (a.detach().double().cpu() - ref.double()).abs().max().item()
    bound = tol * max(1.0, ref.abs().max().item())
    return err <= bound, err, bound


def c3_forward_ref(img, w, bias=None):
    """float64 conv2d(img [B,3,H,W], w [64,3,3,3], bias, stride 1, pad 1) on the CPU."""
    return F.conv2d(img.double().cpu(), w.double().cpu(), None if bias is None else bias.double().cpu(), 1, 1)


def c3_wgrad_ref(img, dy):
    """float64 (dw [64,3,3,3], db [64]) of features.0: img [B,3,H,W], dy [B,64,H,W] (NCHW)."""
    w = torch.zeros((64, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(img.double().cpu(), w, b, 1, 1)
    dw, db = torch.autograd.grad(y, (w, b), dy.double().cpu())
    return dw.detach(), db.detach()


def pool2_ref(x, dy=None):
    """F.max_pool2d(x, 2, 2) in float64 on the CPU and, with dy, its autograd input gradient (both float64)."""
    xr = x.detach().cpu().double().clone().requires_grad_(dy is not None)
    y = F.max_pool2d(xr, 2, 2)
    if dy is None:
        return y.detach()
    y.backward(dy.detach().cpu().double())
    return y.detach(), xr.grad.detach()


def pool_inputs(B, H, W, C, seed):
    """{kind: x [B,C,H,W] f32}: random; post-ReLU (half exact zeros: ties are the common case); every window all equal; the maximum
    planted at window position 0 .. 3 (row-major) of every window, the other three values drawn below it."""
    g = torch.Generator().manual_seed(seed)
    out = {"random": torch.randn((B, C, H, W), generator=g), "relu": torch.relu(torch.randn((B, C, H, W), generator=g))}
    out["equal"] = torch.randn((B, C, H // 2, W // 2), generator=g).repeat_interleave(2, 2).repeat_interleave(2, 3)
    for k in range(4):
        x = -torch.rand((B, C, H, W), generator=g) - 1.0
        x[:, :, k // 2::2, k % 2::2] = torch.rand((B, C, H // 2, W // 2), generator=g)
        out["max at %d" % k] = x
    return out
