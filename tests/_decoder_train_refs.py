"""References and case tables for the training decoder's kernels: csrc/upsample.hip (bilinear, align_corners = True, forward
and adjoint) and csrc/groupnorm.hip (GroupNorm over channel quads + ReLU, forward and backward).  Plain numpy / torch on
the CPU; shared by tests/test_decoder_train_refs_host.py (no GPU) and tests/test_gpu_decoder_train_kernels.py.

Upsample.  src_index and the ratio r are mirrored in float32 bit for bit (one float32 division for r, one float32 product
r * o, a truncation, one subtraction, 1 - l1), so the per-axis weight matrices hold the very float32 weights the kernels
use.  Reference A applies them in float64 (Wy @ x @ Wx^T, and the transposes for the adjoint); reference B is torch's
float64 interpolate and its autograd, which also differs from the kernels by the float32 source coordinate.

Error bar against A (derived, not measured): u = 2^-24, S = |Wy| @ |x| @ |Wx|^T in float64, |got - A| <= gamma_k S with
gamma_k = k u / (1 - k u).
  forward   k = 6: l0 = 1 - l1 is rounded once per axis (2; the matrices hold the same rounded value, which only makes the
            bar generous), and a value goes through lx * v, the row's sum, ly * row and the last sum (4).
  adjoint   a pass is a dot product of n taps taken in order from acc = 0: a term sees its product's rounding and at most
            n - 1 sums, n roundings in all; taps with weight 0 add an exact 0.  The x pass result is stored in float32
            (already counted: the accumulator is float32) and feeds the y pass: k = taps_x + taps_y, the largest number of
            non-zero weights in a column of each axis' matrix (about 2 / r + 1 per axis: up to 10 at scale 4, 5 at scale 2).
"""
import numpy as np
import torch

F32 = np.float32
U24 = 2.0 ** -24
K_UP_FWD = 6
UP_B_RTOL = 2e-5                    # against torch's float64 interpolate: of max(1, |ref|max), as tests/test_gpu_train.py
UP_TAPS = 12                        # kUpTaps of csrc/upsample.hip
UP_PATCH_W, UP_PATCH_H = 34, 4      # kUpPatchW, kUpPatchH


def gamma_k(k):
    return k * U24 / (1.0 - k * U24)


# ---- upsample: the index mirror ------------------------------------------------------------------------------------------


def up_ratio(n_in, n_out):
    return F32(0.0) if n_out <= 1 else F32(F32(n_in - 1) / F32(n_out - 1))


def src_index(r, o, n):
    """The kernels' src_index for an array of output coordinates: i0, i1 (int), l0, l1 (float32)."""
    o = np.asarray(o)
    s = (F32(r) * o.astype(F32)).astype(F32)
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    l0 = (F32(1.0) - l1).astype(F32)
    return i0, i1, l0, l1


def axis_weights(n_in, scale):
    """Dense float32 [n_out, n_in]: row o holds l0 at i0 and l1 at i1 (their float32 sum where i0 == i1, as adjoint_weight)."""
    n_out = n_in * scale
    i0, i1, l0, l1 = src_index(up_ratio(n_in, n_out), np.arange(n_out), n_in)
    W = np.zeros((n_out, n_in), F32)
    rows = np.arange(n_out)
    same = i0 == i1
    W[rows, i0] = np.where(same, (l0 + l1).astype(F32), l0)
    W[rows[~same], i1[~same]] = l1[~same]
    return W


def adjoint_range(n_in, scale):
    """lo, hi of the kernels' adjoint_range for every input coordinate of an axis (float32 arithmetic as there)."""
    n_out = n_in * scale
    r = up_ratio(n_in, n_out)
    i = np.arange(n_in)
    if r > 0:
        lo = np.maximum(0, np.floor(((i - 1).astype(F32) / r).astype(F32)).astype(np.int64) - 1)
        hi = np.minimum(n_out - 1, np.ceil(((i + 1).astype(F32) / r).astype(F32)).astype(np.int64) + 1)
    else:
        lo, hi = np.zeros(n_in, np.int64), np.full(n_in, n_out - 1, np.int64)
    return lo, hi


def rolled_count(n_in, scale):
    """Input coordinates of the axis that take the rolled loop (hi - lo >= kUpTaps), and the largest hi - lo."""
    lo, hi = adjoint_range(n_in, scale)
    return int((hi - lo >= UP_TAPS).sum()), int((hi - lo).max())


def patch_extent(n_in, scale, block):
    """Largest number of source coordinates a block of `block` consecutive outputs reads (k_up_fwd_nhwc_to_nchw: 64 columns,
    4 rows): i1 of the block's last output - i0 of its first + 1."""
    n_out = n_in * scale
    i0, i1, _, _ = src_index(up_ratio(n_in, n_out), np.arange(n_out), n_in)
    first = np.arange(0, n_out, block)
    last = np.minimum(first + block, n_out) - 1
    return int((i1[last] - i0[first] + 1).max())


def taps(n_in, scale):
    return int((axis_weights(n_in, scale) != 0).sum(axis=0).max())


def k_up_bwd(h, w, scale):
    return taps(w, scale) + taps(h, scale)


# ---- upsample: references ----------------------------------------------------------------------------------------------------


def up_forward_A(x, scale):
    """x [B,C,h,w] -> (A, S): the float64 application of the float32 weights and the weighted sum of absolute values."""
    Wy, Wx = axis_weights(x.shape[2], scale).astype(np.float64), axis_weights(x.shape[3], scale).astype(np.float64)
    x = x.astype(np.float64)
    return Wy @ x @ Wx.T, np.abs(Wy) @ np.abs(x) @ np.abs(Wx).T


def up_adjoint_A(g, scale):
    """g [B,C,H,W] -> (A, S) of the adjoint: Wy^T @ g @ Wx."""
    Wy, Wx = axis_weights(g.shape[2] // scale, scale).astype(np.float64), axis_weights(g.shape[3] // scale, scale).astype(np.float64)
    g = g.astype(np.float64)
    return Wy.T @ g @ Wx, np.abs(Wy).T @ np.abs(g) @ np.abs(Wx)


def up_forward_B(x, scale, dtype=torch.float64):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return torch.nn.functional.interpolate(t, scale_factor=scale, mode="bilinear", align_corners=True).numpy()


def up_adjoint_B(g, scale, dtype=torch.float64):
    B, C, H, W = g.shape
    x = torch.zeros((B, C, H // scale, W // scale), dtype=dtype, requires_grad=True)
    y = torch.nn.functional.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=True)
    y.backward(torch.from_numpy(np.ascontiguousarray(g)).to(dtype))
    return x.grad.numpy()


def up_forward_f32(x, scale):
    """The forward kernels' formula, every operation rounded to float32."""
    x = x.astype(F32)
    h, w = x.shape[2:]
    y0, y1, ly0, ly1 = src_index(up_ratio(h, h * scale), np.arange(h * scale), h)
    x0, x1, lx0, lx1 = src_index(up_ratio(w, w * scale), np.arange(w * scale), w)
    top = lx0 * x[:, :, y0][:, :, :, x0] + lx1 * x[:, :, y0][:, :, :, x1]
    bot = lx0 * x[:, :, y1][:, :, :, x0] + lx1 * x[:, :, y1][:, :, :, x1]
    out = ly0[:, None] * top + ly1[:, None] * bot
    assert out.dtype == F32
    return out


def _adjoint_pass_f32(src, n_in, scale):
    """src [..., n_out] float32 -> [..., n_in]: the kernels' tap loop (lo .. hi in order, float32 accumulator)."""
    W = axis_weights(n_in, scale)
    lo, hi = adjoint_range(n_in, scale)
    i = np.arange(n_in)
    acc = np.zeros(src.shape[:-1] + (n_in,), F32)
    for k in range(int((hi - lo).max()) + 1):
        o = np.minimum(lo + k, hi)
        wv = np.where(lo + k <= hi, W[o, i], F32(0.0)).astype(F32)
        acc = acc + wv * src[..., o]
    assert acc.dtype == F32
    return acc


def up_adjoint_f32(g, scale):
    """x pass, result in float32, then y pass, as fpc_upsample_bilinear_bwd."""
    g = g.astype(F32)
    H, W = g.shape[2:]
    tmp = _adjoint_pass_f32(g, W // scale, scale)                                        # [B,C,H,w]
    return np.swapaxes(_adjoint_pass_f32(np.swapaxes(tmp, 2, 3), H // scale, scale), 2, 3)


# ---- upsample: case tables -----------------------------------------------------------------------------------------------------
# forward form codes (fpc_upsample_bilinear_form, backward = 0) and those of a backward pass
FWD_SCALAR, FWD_NHWC4, FWD_LDS, FWD_NCHW4 = 0, 1, 2, 3
BWD_SCALAR, BWD_NHWC4, BWD_NCHW = 0, 1, 2
FWD_FORMS = {FWD_SCALAR, FWD_NHWC4, FWD_LDS, FWD_NCHW4}
BWD_PAIRS = {(BWD_SCALAR, BWD_SCALAR), (BWD_NHWC4, BWD_NHWC4), (BWD_NHWC4, BWD_SCALAR), (BWD_NCHW, BWD_NCHW)}


def src_geometry(spec, B, C, Y, X):
    """Element strides (b, c, y, x) of a [B,C,Y,X] source in the layout `spec`, the offset of its first element inside the
    buffer that holds it (a slice starts past the buffer's start) and the buffer's length, all in floats."""
    kind = spec[0]
    if kind == "nchw":
        st, first = (C * Y * X, Y * X, X, 1), 0
    elif kind == "nhwc":
        st, first = (Y * X * C, 1, X * C, C), 0
    elif kind == "nhwc_slice":                      # channels c0 .. c0 + C of a channel-last tensor with Cw channels
        Cw, c0 = spec[1:]
        st, first = (Y * X * Cw, 1, X * Cw, Cw), c0
    elif kind == "nchw_slice":                      # channels c0 .. c0 + C of an NCHW tensor with Cw channels
        Cw, c0 = spec[1:]
        st, first = (Cw * Y * X, Y * X, X, 1), c0 * Y * X
    elif kind == "nhwc_rowpad":                     # a width slice of a channel-last tensor `pad` pixels wider
        Xw = X + spec[1]
        st, first = (Y * Xw * C, 1, Xw * C, C), 0
    elif kind == "nchw_rowpad":                     # a width slice of an NCHW tensor `pad` columns wider
        Xw = X + spec[1]
        st, first = (C * Y * Xw, Y * Xw, Xw, 1), 0
    elif kind == "plane_c1":                        # one channel, its (arbitrary) stride given as 1: x fastest AND sc == 1
        assert C == 1
        st, first = (Y * X, 1, X, 1), 0
    elif kind == "zero":                            # an expanded scalar: what sum().backward() hands the wrapper
        st, first = (0, 0, 0, 0), 0
    else:
        raise ValueError(kind)
    last = first + sum((n - 1) * s for n, s in zip((B, C, Y, X), st))
    return st, first, last + 1


def scatter_source(values, spec):
    """values [B,C,Y,X] float32 -> (buffer float32 with NaN wherever the source does not live, strides, first)."""
    B, C, Y, X = values.shape
    st, first, n = src_geometry(spec, B, C, Y, X)
    buf = np.full(n, np.nan, F32)
    idx = first + sum(np.arange(m).reshape([-1 if a == k else 1 for a in range(4)]) * s for k, (m, s) in enumerate(zip((B, C, Y, X), st)))
    buf[idx.reshape(-1)] = values.reshape(-1)
    return buf, st, first


def _up(name, B, C, h, w, scale, src, dst_nhwc, form, off=(0, 0, 0), **claims):
    return dict(name=name, B=B, C=C, h=h, w=w, scale=scale, src=src, dst_nhwc=dst_nhwc, form=form, off=off, claims=claims)


# off: pointer offsets in floats (source, destination, scratch) on top of 16-byte aligned buffers.  claims: patch = (rows, columns)
# of the LDS patch; rolled = (x pass, y pass): whether some coordinate of the axis takes the rolled loop.
UP_FWD_CASES = [
    # the LDS form (channel-last -> NCHW, C <= 32)
    _up("lds-s2-full-patch", 2, 7, 7, 70, 2, ("nhwc",), 0, FWD_LDS, patch=(4, 34)),      # 3 column blocks (last: 12), 4 row blocks (last: 2)
    _up("lds-s2-c32", 1, 32, 6, 66, 2, ("nhwc",), 0, FWD_LDS, patch=(4, 34)),
    _up("lds-c1", 2, 1, 5, 9, 4, ("plane_c1",), 0, FWD_LDS, patch=(3, 9)),
    _up("lds-h1", 1, 6, 1, 9, 4, ("nhwc",), 0, FWD_LDS, patch=(1, 9)),
    _up("lds-w1", 1, 5, 6, 1, 2, ("nhwc",), 0, FWD_LDS, patch=(4, 1)),
    _up("lds-s4-unaligned", 1, 3, 5, 17, 4, ("nhwc",), 0, FWD_LDS, off=(1, 3, 0), patch=(3, 17)),
    _up("lds-s4-row-padded", 2, 7, 9, 40, 4, ("nhwc_rowpad", 3), 0, FWD_LDS, patch=(3, 18)),
    _up("c33-falls-to-nchw4", 1, 33, 3, 4, 4, ("nhwc",), 0, FWD_NCHW4),
    # four columns per thread, NCHW destination
    _up("nchw4-two-blocks", 2, 3, 5, 130, 2, ("nchw",), 0, FWD_NCHW4),                   # W / 4 = 65, H = 10
    _up("nchw4-nchw-slice", 2, 3, 3, 8, 4, ("nchw_slice", 5, 1), 0, FWD_NCHW4),
    _up("nchw4-nhwc-slice", 1, 3, 4, 6, 2, ("nhwc_slice", 8, 4), 0, FWD_NCHW4),
    # four channels per thread, channel-last on both sides
    _up("nhwc4-two-blocks", 2, 128, 3, 5, 2, ("nhwc",), 1, FWD_NHWC4),                   # W C / 4 = 320
    _up("nhwc4-s4", 1, 12, 5, 7, 4, ("nhwc",), 1, FWD_NHWC4),
    _up("nhwc4-slice", 2, 8, 3, 4, 2, ("nhwc_slice", 16, 4), 1, FWD_NHWC4),
    _up("nhwc4-from-nchw", 1, 4, 3, 5, 2, ("nchw",), 1, FWD_SCALAR),                      # sc != 1
    # one element per thread, each way in
    _up("scalar-unaligned-nchw", 1, 3, 3, 4, 2, ("nchw",), 0, FWD_SCALAR, off=(0, 1, 0)),
    _up("scalar-unaligned-nhwc", 2, 8, 3, 40, 4, ("nhwc",), 1, FWD_SCALAR, off=(2, 0, 0)),   # 2 blocks along (x, c)
    _up("scalar-strides", 1, 4, 4, 3, 2, ("nhwc_slice", 5, 1), 1, FWD_SCALAR),
    _up("scalar-w-odd", 3, 5, 3, 5, 2, ("nchw",), 0, FWD_SCALAR),
    _up("scalar-w-odd-blocks", 1, 2, 9, 17, 2, ("nchw",), 0, FWD_SCALAR),                 # 18 x 34 = 612 elements per plane
    _up("scalar-c6-nhwc", 2, 6, 2, 3, 4, ("nhwc",), 1, FWD_SCALAR),
]

UP_BWD_CASES = [
    # channel-last gradient, four channels per thread in both passes
    _up("cc-s4", 2, 8, 5, 6, 4, ("nhwc",), 1, (BWD_NHWC4, BWD_NHWC4), rolled=(True, True)),
    _up("cc-s2-two-blocks", 1, 128, 3, 9, 2, ("nhwc",), 1, (BWD_NHWC4, BWD_NHWC4), rolled=(False, False)),
    _up("cc-s4-tiny", 1, 4, 4, 3, 4, ("nhwc",), 1, (BWD_NHWC4, BWD_NHWC4), rolled=(False, False)),
    _up("cc-slice", 2, 8, 5, 5, 4, ("nhwc_slice", 12, 4), 1, (BWD_NHWC4, BWD_NHWC4), rolled=(True, True)),
    # channel-last gradient, NCHW input gradient: the y pass is the scalar kernel in channel order on NCHW strides
    _up("cs-s4", 1, 4, 6, 5, 4, ("nhwc",), 0, (BWD_NHWC4, BWD_SCALAR), rolled=(True, True)),
    _up("cs-s2", 2, 8, 3, 4, 2, ("nhwc",), 0, (BWD_NHWC4, BWD_SCALAR), rolled=(False, False)),
    # x-fastest gradient
    _up("xx-s4", 2, 3, 5, 8, 4, ("nchw",), 0, (BWD_NCHW, BWD_NCHW), rolled=(True, True)),
    _up("xx-s2-row-tail", 1, 2, 5, 68, 2, ("nchw",), 0, (BWD_NCHW, BWD_NCHW), rolled=(False, False)),      # H = 10, two column blocks
    _up("xx-s4-tiny", 2, 2, 3, 4, 4, ("nchw",), 0, (BWD_NCHW, BWD_NCHW), rolled=(False, False)),
    _up("xx-s4-to-nhwc", 1, 3, 5, 8, 4, ("nchw",), 1, (BWD_NCHW, BWD_NCHW), rolled=(True, True)),
    _up("xx-slice", 2, 3, 3, 8, 2, ("nchw_slice", 5, 1), 0, (BWD_NCHW, BWD_NCHW), rolled=(False, False)),
    # one element per thread in both passes
    _up("ss-unaligned-nchw-s4", 2, 3, 5, 8, 4, ("nchw",), 0, (BWD_SCALAR, BWD_SCALAR), off=(0, 0, 1), rolled=(True, True)),
    _up("ss-unaligned-nhwc-s2", 1, 8, 3, 5, 2, ("nhwc",), 1, (BWD_SCALAR, BWD_SCALAR), off=(3, 0, 0), rolled=(False, False)),
    _up("ss-zero-strides-s4", 2, 3, 6, 5, 4, ("zero",), 0, (BWD_SCALAR, BWD_SCALAR), rolled=(True, True)),
    _up("ss-zero-strides-s2", 2, 3, 4, 5, 2, ("zero",), 1, (BWD_SCALAR, BWD_SCALAR), rolled=(False, False)),
    _up("ss-w-odd-to-nhwc", 1, 3, 5, 7, 4, ("nchw",), 1, (BWD_SCALAR, BWD_SCALAR), rolled=(True, True)),
    _up("ss-c6-nhwc-to-nchw", 2, 6, 7, 9, 4, ("nhwc",), 0, (BWD_SCALAR, BWD_SCALAR), rolled=(True, True)),  # 2 blocks in the x pass
    _up("ss-strides", 1, 4, 3, 4, 2, ("nhwc_slice", 5, 1), 1, (BWD_SCALAR, BWD_SCALAR), rolled=(False, False)),
    _up("ss-row-padded", 1, 2, 3, 4, 2, ("nchw_rowpad", 1), 0, (BWD_SCALAR, BWD_SCALAR), rolled=(False, False)),
]

# the kernels of each pass by form code: every one needs a case that takes the rolled loop and one that never does
BWD_KERNELS = {(1, BWD_SCALAR): "k_up_bilinear_bwd_1d<0>", (1, BWD_NHWC4): "k_up_bwd_1d_nhwc4<0>", (1, BWD_NCHW): "k_up_bwd_x_nchw",
               (2, BWD_SCALAR): "k_up_bilinear_bwd_1d<1>", (2, BWD_NHWC4): "k_up_bwd_1d_nhwc4<1>", (2, BWD_NCHW): "k_up_bwd_y_nchw4"}


def up_case_id(case):
    return case["name"]


def up_values(case, backward):
    """The logical source of a case, float32 [B,C,.,.]: the input of the forward or the output gradient of the backward."""
    B, C, h, w, s = (case[k] for k in ("B", "C", "h", "w", "scale"))
    shape = (B, C, h * s, w * s) if backward else (B, C, h, w)
    seed = sum(ord(ch) for ch in case["name"]) + (1000 if backward else 0)
    if case["src"][0] == "zero":
        return np.full(shape, F32(0.8125), F32)
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def up_low4(case, backward, extra=0):
    """Low four bits of the pointers of a case on 16-byte aligned buffers, or-ed (the scratch only in the backward)."""
    B, C, h, w, s = (case[k] for k in ("B", "C", "h", "w", "scale"))
    _, first, _ = src_geometry(case["src"], B, C, h * s if backward else h, w * s if backward else w)
    offs = [first + case["off"][0] + extra, case["off"][1] + extra] + ([case["off"][2] + extra] if backward else [])
    bits = 0
    for o in offs:
        bits |= (4 * o) & 15
    return bits


def forced_scalar(case, backward):
    """The same data on the one-element-per-thread kernels: every pointer a float off 16-byte alignment and, for the LDS
    form (which asks for no alignment), the source as a channel slice of a tensor one channel wider."""
    c = dict(case)
    c["off"] = (1, 1, 1)
    if not backward and case["form"] == FWD_LDS:
        c["src"] = ("nhwc_slice", case["C"] + 1, 0) if case["C"] > 1 else ("nchw_rowpad", 1)
        c["off"] = (0, 1, 0)
    c["form"] = (BWD_SCALAR, BWD_SCALAR) if backward else FWD_SCALAR
    c["name"] = case["name"] + "-forced"
    return c


# ---- GroupNorm + ReLU ------------------------------------------------------------------------------------------------------------
GN_CHUNK = 256                      # kGnChunk of csrc/groupnorm.hip
GN_Y_RTOL, GN_GRAD_RTOL = 2e-5, 1e-4          # of max(1, |ref|max), as tests/test_gpu_train.py
GN_MEAN_RTOL, GN_RSTD_RTOL, GN_RSTD_RTOL_OFFSET = 1e-6, 1e-5, 2e-3
GN_Z_EDGE, GN_EDGE_CAP = 1e-4, 1e-3

# (B, C, H, W, groups, eps, input kind)
GN_CASES = [
    (2, 4, 1, 1, 1, 1e-5, "randn"),
    (1, 8, 1, 3, 2, 1e-3, "randn"),
    (2, 16, 15, 17, 4, 1e-5, "randn"),             # HW = 255
    (1, 32, 16, 16, 8, 1e-3, "randn"),             # HW = 256
    (2, 64, 1, 257, 16, 1e-5, "randn"),            # a one-pixel tail chunk
    (1, 128, 27, 19, 32, 1e-3, "randn"),           # HW = 513
    (1, 256, 10, 103, 64, 1e-5, "randn"),          # HW Q = 65 920: the grid-stride loops of the elementwise kernels wrap
    (2, 128, 1, 257, 32, 1e-5, "offset"),          # 100 + 0.05 randn, two chunks, a one-pixel tail
    (1, 16, 1, 257, 4, 1e-5, "constant"),          # group 1 is exactly constant
    (2, 16, 3, 5, 4, 1e-3, "constant"),
]


def gn_case_id(case):
    return "-".join(str(v) for v in case)


def _offset_input(rng, B, HW, Q):
    """100 + 0.05 randn stated on the grid 2^-10, with every sum the kernel rounds to float32 exactly representable, so that the
    float32 statistics are the float64 ones: per (image, group) each full chunk's sum is a multiple of 2^-7 (the float32 grid at
    ~102 400) and the group's mean a multiple of 2^-17 (the float32 grid at ~100).  The kernel's per-thread float32 sums are exact
    too (at most 128 values of ~100 on the 2^-10 grid: below 2^24 grid steps) for groups <= 32."""
    assert HW == GN_CHUNK + 1 and Q <= 32
    k = np.rint(rng.standard_normal((B, HW, Q, 4)) * (0.05 * 1024)).astype(np.int64)
    k[:, GN_CHUNK - 1, :, 3] -= k[:, :GN_CHUNK].sum(axis=(1, 3)) % 8
    n = 4 * HW                                                               # 1028 = 4 * 257: the mean's grid asks for 257 | sum k
    t = (-k[:, :GN_CHUNK].sum(axis=(1, 3))) % (n // 4)
    t = np.where(t > n // 8, t - n // 4, t)
    k[:, GN_CHUNK] = t[..., None] // 4
    k[:, GN_CHUNK, :, 0] += t - 4 * (t // 4)
    assert (k.sum(axis=(1, 3)) % (n // 4) == 0).all() and (k[:, :GN_CHUNK].sum(axis=(1, 3)) % 8 == 0).all()
    x = (100.0 + k / 1024.0).astype(F32)
    assert (x.astype(np.float64) == 100.0 + k / 1024.0).all()
    return x.reshape(B, HW, 4 * Q)


def gn_inputs(case):
    """x, dy [B,HW,C], gamma, beta [C], all float32.  gamma has both signs and gamma[1] == 0; |beta| stays above the ReLU edge."""
    B, C, H, W, Q, eps, kind = case
    HW = H * W
    rng = np.random.default_rng(C * 1000 + HW * 7 + B)
    if kind == "offset":
        x = _offset_input(rng, B, HW, Q)
    else:
        x = (rng.standard_normal((B, HW, C)) * 1.5 + 0.7).astype(F32)
        if kind == "constant":
            x[0, :, 4:8] = F32(0.75)
    dy = rng.standard_normal((B, HW, C)).astype(F32)
    gamma = ((rng.random(C) + 0.5) * np.where(np.arange(C) % 3 == 2, -1.0, 1.0)).astype(F32)
    gamma[1] = 0.0
    beta = (rng.standard_normal(C) * 0.3).astype(F32)
    beta = np.where(np.abs(beta) < 0.01, F32(0.05), beta).astype(F32)
    return x, dy, gamma, beta


def gn_forward_ref(x, gamma, beta, Q, eps, dtype=np.float64):
    """y, z (the pre-activation), mean [B,Q], rstd [B,Q], xhat.  dtype float32 evaluates the kernels' formulas with every
    elementwise operation rounded to float32 (the statistics are float64 sums rounded once, as the kernels store them)."""
    B, HW, C = x.shape
    xg = x.astype(np.float64).reshape(B, HW, Q, 4)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + np.float64(F32(eps)))
    mean, rstd = mean.astype(dtype), rstd.astype(dtype)
    g, b = gamma.astype(dtype), beta.astype(dtype)
    xhat = ((x.astype(dtype).reshape(B, HW, Q, 4) - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, HW, C)
    z = xhat * g + b
    assert z.dtype == dtype
    return np.maximum(z, dtype(0)), z, mean, rstd, xhat


def gn_backward_ref(x, dy, gamma, beta, Q, eps, mask, dtype=np.float64):
    """dx [B,HW,C], dgamma, dbeta [C] and the per-chunk table [B][chunks][C][2] = {sum dz, sum dz xhat} for a given ReLU mask.
    dtype float32: the kernels' formulas in float32, the sums taken in float64 over float32 terms and rounded once."""
    B, HW, C = x.shape
    _, _, mean, rstd, xhat = gn_forward_ref(x, gamma, beta, Q, eps, dtype)
    g = gamma.astype(dtype)
    dz = np.where(mask, dy.astype(dtype), dtype(0))
    chunks = -(-HW // GN_CHUNK)
    part = np.zeros((B, chunks, C, 2), dtype)
    dzx = dz * xhat
    for k in range(chunks):
        sl = slice(k * GN_CHUNK, min(HW, (k + 1) * GN_CHUNK))
        part[:, k, :, 0] = dz[:, sl].astype(np.float64).sum(axis=1).astype(dtype)
        part[:, k, :, 1] = dzx[:, sl].astype(np.float64).sum(axis=1).astype(dtype)
    sums = part.astype(np.float64).sum(axis=(0, 1))
    per_image = part.astype(np.float64).sum(axis=1)                                       # [B,C,2]
    n = 4.0 * HW
    m1 = ((per_image[:, :, 0] * g.astype(np.float64)).reshape(B, Q, 4).sum(axis=2) / n).astype(dtype)
    m2 = ((per_image[:, :, 1] * g.astype(np.float64)).reshape(B, Q, 4).sum(axis=2) / n).astype(dtype)
    rep = lambda v: np.repeat(v, 4, axis=1)[:, None, :]                                   # [B,Q] -> [B,1,C]
    dx = rep(rstd) * (dz * g - rep(m1) - xhat * rep(m2))
    assert dx.dtype == dtype
    return dx, sums[:, 1], sums[:, 0], part


def gn_torch_ref(x, dy, gamma, beta, H, W, Q, eps, mask=None):
    """torch.nn.GroupNorm(...).double() + ReLU and its autograd on the same numbers: y, dx [B,HW,C], dgamma, dbeta.  With a
    mask the ReLU's derivative is replaced by it."""
    B, HW, C = x.shape
    gn = torch.nn.GroupNorm(Q, C, eps=float(F32(eps))).double()
    gn.weight.data, gn.bias.data = torch.from_numpy(gamma).double(), torch.from_numpy(beta).double()
    xt = torch.from_numpy(x).double().reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_()
    dyt = torch.from_numpy(dy).double().reshape(B, H, W, C).permute(0, 3, 1, 2)
    z = gn(xt)
    if mask is None:
        y = torch.relu(z)
        y.backward(dyt)
    else:
        y = z * torch.from_numpy(mask).double().reshape(B, H, W, C).permute(0, 3, 1, 2)
        y.backward(dyt)
    back = lambda t: t.detach().permute(0, 2, 3, 1).reshape(B, HW, C).numpy()
    return back(y), back(xt.grad), gn.weight.grad.numpy(), gn.bias.grad.numpy()
