"""Float64 references for the training-side kernels of csrc/train.hip: plain numpy and torch on the CPU, no GPU code and no
test functions.  tests/test_train_refs_host.py checks these references themselves (against lib/loss.py in float64, against
autograd and against the CPU oracle's thinning); tests/test_gpu_train_kernels.py holds the kernels to them.

Every function that takes `dtype` evaluates the same formulas in that precision: float64 is the reference, float32 is the
"torch-op form" whose own rounding error the tests' tolerances are measured against.
"""
import math

import numpy as np
import torch

# ---- mask losses (k_mask_losses) ----------------------------------------------------------------------------------------


def _mask_loss_terms(x, target, ignore_ce, ignore_cce, alpha, gamma):
    """(CE sum, CE count, CCE sum, CCE count, Focal sum, Focal count) as 0-dim tensors of x's dtype, by the formulas of the
    kernel's header comment.  x [B,C,HW], target i64 [B,HW].  A target outside [0, C) adds nothing to CE / CCE and is not
    counted there (lib/loss.py:_fused_mask_loss); Focal sees it as "no positive class" unless it is the ignore value."""
    C = x.shape[1]
    y = torch.log_softmax(x, dim=1)
    in_range = (target >= 0) & (target < C)
    ce_on = in_range & (target != ignore_ce)
    cce_on = in_range & (target != ignore_cce)
    foc_on = target != ignore_cce
    picked = torch.gather(y, 1, target.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    zero = torch.zeros((), dtype=x.dtype)
    ce = -torch.where(ce_on, picked, zero).sum()
    cce = -torch.where(cce_on, picked, zero).sum()
    tgt = (target.unsqueeze(1) == torch.arange(C).view(1, C, 1)).to(x.dtype)
    bce = y.clamp(min=0) - y * tgt + torch.log1p(torch.exp(-y.abs()))
    pt = torch.exp(-bce)
    a = alpha * tgt + (1.0 - alpha) * (1.0 - tgt)
    focal = torch.where(foc_on.unsqueeze(1), a * (1.0 - pt).pow(gamma) * bce, zero).sum()
    cnt = [m.sum().to(x.dtype) for m in (ce_on, cce_on, foc_on)]
    return ce, cnt[0], cce, cnt[1], focal, cnt[2]


def _as3(logits, target):
    x = torch.as_tensor(logits)
    t = torch.as_tensor(target).to(torch.int64)
    return x.reshape(x.shape[0], x.shape[1], -1), t.reshape(t.shape[0], -1)


def mask_losses_ref(logits, target, ignore_ce, ignore_cce, alpha, gamma, dtype=torch.float64):
    """The six sums and counts of fpc_mask_losses' `sums6`, as a numpy float64 [6]."""
    x, t = _as3(logits, target)
    with torch.no_grad():
        out = _mask_loss_terms(x.to(dtype), t, ignore_ce, ignore_cce, alpha, gamma)
    return np.array([float(v) for v in out], np.float64)


def mask_losses_grad_ref(logits, target, ignore_ce, ignore_cce, alpha, gamma, w3, dtype=torch.float64):
    """d(w0 CEsum + w1 CCEsum + w2 Focalsum) / d logits by torch autograd, in the logits' shape.  No reference exists for
    gamma < 1: the derivative of (1 - pt)^gamma is infinite where 1 - pt rounds to 0."""
    x, t = _as3(logits, target)
    x = x.to(dtype).clone().requires_grad_(True)
    ce, _, cce, _, focal, _ = _mask_loss_terms(x, t, ignore_ce, ignore_cce, alpha, gamma)
    (float(w3[0]) * ce + float(w3[1]) * cce + float(w3[2]) * focal).backward()
    return x.grad.reshape(torch.as_tensor(logits).shape)


# ---- class compression (k_cc_backward) ----------------------------------------------------------------------------------
CC_HEADS = (("quaternion", 4, True), ("scales", 3, False), ("xy", 2, True), ("z", 1, False))   # key, channels per class, normalised


def class_compress_ref(C, cat_mask, logits):
    """Gather of each pixel's class group, then x / |x| for quaternion and xy (identity where |x| == 0), in the dtype of
    `logits`; background and class ids outside [1, C) give zeros.  logits[key]: [B, a (C - 1), HW]; returns [B, a, HW]."""
    fg = (cat_mask >= 1) & (cat_mask < C)
    grp = torch.where(fg, cat_mask - 1, torch.zeros_like(cat_mask))
    out = {}
    for key, a, norm in CC_HEADS:
        v = logits[key]
        idx = grp.unsqueeze(1) * a + torch.arange(a).view(1, a, 1)
        sel = torch.gather(v, 1, idx) * fg.unsqueeze(1).to(v.dtype)
        if norm:
            n2 = (sel * sel).sum(dim=1, keepdim=True)
            sel = sel / torch.sqrt(torch.where(n2 > 0, n2, torch.ones_like(n2)))
        out[key] = sel
    return out


def class_compress_backward_ref(C, cat_mask, logits, go, dtype=torch.float64):
    """d sum_k <class_compress(logits)[k], go[k]> / d logits[k] by autograd; go[key] may be None (that head gets zeros)."""
    leaves = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in logits.items()}
    out = class_compress_ref(C, cat_mask, leaves)
    total = sum((out[k] * torch.as_tensor(go[k]).to(dtype)).sum() for k in out if go.get(k) is not None)
    grads = {k: torch.zeros_like(v) for k, v in leaves.items()}
    if torch.is_tensor(total) and total.requires_grad:
        total.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return grads


# ---- the vote's refinement (k_post_backward, k_vote_refine_backward) ----------------------------------------------------


def refine_solve_torch(d, coords):
    """x = solve(sum n n^T, sum n (n . p)), n = (dy, -dx), over the rows of d [k,2] / coords [k,2] (torch, differentiable)."""
    normal = torch.stack([d[:, 1], -d[:, 0]], dim=1)
    bb = (normal * coords).sum(dim=1)
    return torch.linalg.solve(normal.T @ normal, (normal * bb[:, None]).sum(dim=0))


def refine_grad_autograd(d, coords, g):
    """d <x, g> / d d for the refinement over the given pixel set, float64 autograd.  d, coords: numpy [k,2]."""
    dd = torch.from_numpy(np.asarray(d, np.float64)).clone().requires_grad_(True)
    x = refine_solve_torch(dd, torch.from_numpy(np.asarray(coords, np.float64)))
    (x * torch.from_numpy(np.asarray(g, np.float64))).sum().backward()
    return x.detach().numpy(), dd.grad.numpy()


def normal_matrix(d, coords):
    """(a00, a01, a11, b0, b1) of the normal equations over the set, numpy float64."""
    d, coords = np.asarray(d, np.float64), np.asarray(coords, np.float64)
    nx, ny = d[:, 1], -d[:, 0]
    bb = nx * coords[:, 0] + ny * coords[:, 1]
    return (nx * nx).sum(), (nx * ny).sum(), (ny * ny).sum(), (nx * bb).sum(), (ny * bb).sum()


def solve2_sym(a00, a01, a11, b0, b1):
    """csrc/ransac.hip:solve2_sym restated: the inverse when det > 1e-12 tr^2, else the documented singular rule
    x = A b / tr^2, and (0, 0) when tr <= 0."""
    tr, det = a00 + a11, a00 * a11 - a01 * a01
    if not tr > 0.0:
        return 0.0, 0.0
    if det <= 1e-12 * tr * tr:
        s = 1.0 / (tr * tr)
        return (a00 * b0 + a01 * b1) * s, (a01 * b0 + a11 * b1) * s
    inv = 1.0 / det
    return (a11 * b0 - a01 * b1) * inv, (-a01 * b0 + a00 * b1) * inv


def refine_grad(coords, d, x, lam):
    """The native per-pixel formula (csrc/train.hip:refine_grad) in numpy float64: rows (dL/d dx, dL/d dy) for pixels at
    `coords` [k,2] with directions d [k,2], refined point x and lam = (sum n n^T)^-1 dL/dx."""
    coords, d = np.asarray(coords, np.float64), np.asarray(d, np.float64)
    nx, ny = d[:, 1], -d[:, 0]
    rx, ry = coords[:, 0] - x[0], coords[:, 1] - x[1]
    r = nx * rx + ny * ry
    ln = lam[0] * nx + lam[1] * ny
    gnx, gny = lam[0] * r + ln * rx, lam[1] * r + ln * ry
    return np.stack([-gny, gnx], axis=1)


# ---- thinning (include/fpc_rng.h) ---------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(h):
    h = h.astype(np.uint64)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85ebca6b)) & _M32
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xc2b2ae35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def hash3(seed, a, b, c):
    """fpc_hash3 on arrays (uint32 arithmetic carried in uint64 words)."""
    seed = int(seed) & (2 ** 64 - 1)
    a, b, c = (np.asarray(v, dtype=np.uint64) & _M32 for v in (a, b, c))
    h = _mix32(np.uint64((seed & 0xFFFFFFFF) ^ 0x9e3779b9) + np.zeros(np.broadcast(a, b, c).shape, np.uint64))
    h = _mix32(h ^ np.uint64(seed >> 32))
    h = _mix32(h ^ ((a * np.uint64(0x9e3779b1) + np.uint64(0x7f4a7c15)) & _M32))
    h = _mix32(h ^ ((b * np.uint64(0x85ebca77) + np.uint64(0x165667b1)) & _M32))
    h = _mix32(h ^ ((c * np.uint64(0xc2b2ae3d) + np.uint64(0x27d4eb2f)) & _M32))
    return h


def rand_keep(seed, inst, pixel, fg, max_num):
    """fpc_rand_keep on arrays of pixel indices: keep iff r * fg < max_num * 2^32 (both sides below 2^64)."""
    r = hash3(seed, inst, pixel, 0xfeed)
    return (r * np.uint64(fg)) < (np.uint64(max_num) << np.uint64(32))


def kept_mask(seed, inst, mask_flat, max_num):
    """The pixels of one instance the vote fits: all of them up to max_num, else the rand_keep selection (bool [HW])."""
    mask_flat = np.asarray(mask_flat) != 0
    fg = int(mask_flat.sum())
    if fg <= max_num:
        return mask_flat.copy()
    return mask_flat & rand_keep(seed, inst, np.arange(mask_flat.size), fg, max_num)


def inlier_mask(oracle, d32, W, winner, thresh, sel):
    """Inliers of `winner` among the pixels `sel` (bool [HW]) by the oracle's own float32 angle test (bit-identical to the
    kernels'), as a bool [HW].  d32: float32 [2,HW] directions exactly as the kernel reads them."""
    sel = np.asarray(sel, bool)
    out = np.zeros(sel.size, bool)
    idx = np.nonzero(sel)[0]
    if idx.size == 0:
        return out
    coords = np.stack([idx % W, idx // W], axis=1).astype(np.float32)
    direct = np.ascontiguousarray(np.asarray(d32, np.float32)[:, idx].T[:, None, :])
    inl = np.zeros((1, 1, idx.size), np.uint8)
    oracle.voting_for_hypothesis(direct, coords, np.asarray(winner, np.float32).reshape(1, 1, 2), inl, thresh)
    out[idx] = inl[0, 0] != 0
    return out


# ---- optimiser ----------------------------------------------------------------------------------------------------------


def radam_sma(beta2, step):
    """RAdam's length of the approximated simple moving average at `step` (Liu et al. 2020); rectified when >= 5."""
    b2t = beta2 ** step
    return 2 / (1 - beta2) - 1 - 2 * step * b2t / (1 - b2t)


def radam_lookahead_reference(p, grads, lr, betas, eps, wd, k, alpha):
    """catalyst.contrib.nn.RAdam + Lookahead (published algorithms; Liu et al. 2020, Zhang et al. 2019) in float64."""
    p = p.clone().double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    slow = None
    b1, b2 = betas
    for step, g in enumerate(grads, start=1):
        g = g.double()
        v = v * b2 + (1 - b2) * g * g
        m = m * b1 + (1 - b1) * g
        b2t = b2 ** step
        sma_max = 2 / (1 - b2) - 1
        sma = sma_max - 2 * step * b2t / (1 - b2t)
        if wd:
            p = p + (-wd * lr) * p
        if sma >= 5:
            ss = lr * math.sqrt((1 - b2t) * (sma - 4) / (sma_max - 4) * (sma - 2) / sma * sma_max / (sma_max - 2)) / (1 - b1 ** step)
            p = p - ss * m / (v.sqrt() + eps)
        else:
            p = p - lr / (1 - b1 ** step) * m
        if (step - 1) % k == 0:
            if slow is None:
                slow = p.clone()
            slow = slow + (p - slow) * alpha
            p = slow.clone()
    return p


# ---- shared inputs: the same arrays on every machine, built on the host from the case itself -------------------------------
# (C, HW, B, logit spread or "equal", alpha, gamma, target kind).  A reduced cross product: every C with the HW that wraps
# the forward's 96-workgroup grid (24 577), both instantiations (C <= 8 / C > 8) at every spread, every (alpha, gamma) pair,
# HW = 262 145 (wraps the backward's 1024-workgroup grid) for C = 2, B = 1 only.
MASK_LOSS_CASES = [
    (2, 1, 1, 3, 0.5, 2.0, "mixed"),
    (2, 255, 3, 20, 0.25, 2.0, "oor"),
    (2, 24577, 1, 60, 0.25, 1.5, "mixed"),
    (2, 262145, 1, 3, 0.25, 1.0, "oor"),
    (7, 257, 3, 60, 0.5, 2.0, "oor"),
    (7, 24577, 1, 20, 0.25, 1.5, "mixed"),
    (8, 255, 1, 3, 0.25, 1.0, "oor"),
    (8, 24577, 3, 20, 0.5, 2.0, "mixed"),
    (9, 257, 1, 20, 0.25, 2.0, "oor"),
    (9, 24577, 1, 3, 0.25, 1.5, "mixed"),
    (32, 1, 3, 60, 0.25, 1.0, "oor"),
    (32, 24577, 1, 3, 0.5, 2.0, "oor"),
    (32, 255, 1, 60, 0.25, 1.5, "mixed"),
    (7, 255, 1, "equal", 0.5, 2.0, "mixed"),
    (7, 257, 1, 3, 0.5, 2.0, "all-1"),
    (9, 257, 3, 20, 0.25, 1.5, "all-100"),
    # gamma < 1: forward sums against the reference, gradient only finite (no autograd reference exists)
    (9, 255, 1, 60, 0.25, 0.5, "mixed"),
    (7, 24577, 1, 20, 0.5, 0.5, "oor"),
]
MASK_SUM_RTOL = 2e-6        # of max(|sum|, its count): the bar of test_fused_mask_losses_match_torch_forms on the means
MASK_GRAD_RTOL = 2e-5       # of the largest gradient magnitude
CC_RTOL = 2e-6              # of each tensor's largest gradient magnitude
MASK_LOSS_W3 = ((5.0, 3.0, 7.0), (-0.75, 2.5e-3, 0.0625))


def mask_loss_inputs(case):
    """(logits f32 [B,C,HW], target i64 [B,HW]) of one MASK_LOSS_CASES entry."""
    C, HW, B, sigma, _alpha, _gamma, kind = case
    g = torch.Generator().manual_seed(1000 * C + HW % 997 + 7 * B)
    if sigma == "equal":
        x = torch.full((B, C, HW), 1.25)
    else:
        x = torch.randn((B, C, HW), generator=g) * float(sigma)
    t = torch.randint(0, C, (B, HW), generator=g)
    u = torch.rand((B, HW), generator=g)
    if kind == "all-1":
        t[:] = -1
    elif kind == "all-100":
        t[:] = -100
    else:
        t[u < 0.10] = -1
        t[(u >= 0.10) & (u < 0.18)] = -100
        if kind == "oor":
            for k, v in enumerate((C, C + 5, -7, 2 ** 40)):
                t[(u >= 0.18 + 0.04 * k) & (u < 0.22 + 0.04 * k)] = v
            if HW == 1:                                  # one pixel per plane: make sure an out-of-range value is there
                t[0, 0] = C + 5
    return x, t


CC_CASES = [(2, 1, 2), (2, 257, 1), (7, 255, 2), (7, 1000, 1), (32, 257, 1), (32, 1000, 2)]      # C, HW, B


def cc_inputs(case):
    """(cat_mask i64 [B,HW], logits dict f32 [B, a (C-1), HW], go dict f32 [B, a, HW]) of one CC_CASES entry: every class
    and background present (HW permitting), class ids C, -1 and 2^33, norms of the selected vectors in [1e-3, 1e3] (far from
    f32 underflow of |x|^2), a few exactly-zero selected quaternions and a few exactly-zero selected xy."""
    C, HW, B = case
    G = C - 1
    g = torch.Generator().manual_seed(100 * C + HW + B)
    cat = torch.randint(0, C, (B, HW), generator=g)
    if HW >= C:
        cat[:, :C] = torch.arange(C)
    if HW >= 64:
        cat[:, 40], cat[:, 41], cat[:, 42] = C, -1, 2 ** 33
        cat[:, 50:56] = 1 + torch.arange(6) % G
    else:
        cat[0, 0] = G
        cat[-1, -1] = C if HW == 1 and B > 1 else cat[-1, -1]
    logits, go = {}, {}
    for key, a, norm in CC_HEADS:
        v = torch.randn((B, G, a, HW), generator=g)
        if norm:
            v = v / v.norm(dim=2, keepdim=True) * 10.0 ** (torch.rand((B, G, 1, HW), generator=g) * 6.0 - 3.0)
        logits[key] = v
        go[key] = torch.randn((B, a, HW), generator=g)
    if HW >= 64:                                         # zero vectors in the SELECTED group only
        for p in (50, 51, 52):
            logits["quaternion"][:, (cat[0, p] - 1), :, p] = 0.0
        for p in (53, 54, 55):
            logits["xy"][:, (cat[0, p] - 1), :, p] = 0.0
    logits = {k: v.reshape(B, -1, HW).contiguous() for k, v in logits.items()}
    return cat, logits, go


def vote_scene(H, W, seed=0, noise=0.03, pattern=(1, 1, 1, 2, 3, 4, 10, 0, 1, 3)):
    """A label plane with instances 1..3 (plus labels 4 and 10, above N = 3) and unit directions towards one centre per
    label with angular noise, for the crafted-table tests.  labels i32 [HW], d f32 [2,HW], centres f64 [11,2]."""
    HW = H * W
    rng = np.random.default_rng(seed + 31 * H + W)
    p = np.arange(HW)
    labels = np.asarray(pattern, np.int32)[(p * len(pattern)) // HW] if HW > 1 else np.ones(1, np.int32)
    centres = np.stack([rng.uniform(0, W, 11), rng.uniform(0, H, 11)], axis=1) + 0.37
    cx, cy = centres[labels, 0], centres[labels, 1]
    ang = np.arctan2(cy - p // W, cx - p % W) + rng.normal(0, noise, HW)
    d = np.stack([np.cos(ang), np.sin(ang)]).astype(np.float32)
    d[:, labels == 0] = 0.0
    return labels, d, centres
