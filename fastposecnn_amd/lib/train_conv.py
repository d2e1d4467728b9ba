"""Convolutions of the TRAINING step on the native kernels (BASELINE.json configs[4]).

The reference trains through torch.nn.Conv2d, i.e. cuDNN forward and backward under autograd
(F/lib/pose_regressor.py:709-743 inside Lightning's training_step).  Here a convolution in training mode is one
autograd.Function over three native pieces, all on channel-last (NHWC) activations:

  forward        fpc_conv2d: the inference engine's implicit-GEMM / Winograd kernels (csrc/net_kernels.hip), bias fused
  data gradient  stride 1: the SAME kernels on the flipped, transposed weights (a convolution of dy);
                 stride 2 (three encoder convolutions, their 1x1 shortcuts): the same kernels once per output parity
                 (round 4: dx[2a + r] only sees the taps of parity r — 1, 2, 2 and 4 of a 3x3 kernel's nine — so four small
                 stride-1 convolutions of dy write the four interleaved quarter planes; no zero-insertion, 13/9 of the
                 minimal multiply-adds);  heads whose width is not a multiple of 32: dy and W zero-padded to 32 channels
  weight gradient  fpc_conv2d_wgrad (csrc/conv_wgrad.hip): pixels-as-K GEMM on the f32 matrix cores, fixed-order
                 split over the pixels; a width that is not a multiple of 4 (mask / scales / xyz heads) is padded likewise
A GROUPED 3x3 convolution (conv2 of the ResNeXt blocks) is torch's own by default; with FPC_TRAIN_NATIVE_GROUPED=1 it is
_GroupedConv2dFn: k_conv3x3_grouped forward, the same kernel on the in-group transposed, flipped weights (stride 1) or
k_conv3x3_grouped_dgrad_s2 (stride 2) for the data gradient, k_conv3x3_grouped_wgrad for the weight gradient
(csrc/conv_grouped_train.hip) — plain f32 products, one form, nothing tuned.
The 7x7 stem (Cin = 3) is torch's own by default, forward and backward: its input needs no gradient and its weight gradient is a
K = 147 GEMM no tile of the kernels above fits (counted neither as native nor as aten below).  With FPC_TRAIN_NATIVE_STEM=1 it
is _StemConvFn — the image repacked to NHWC4 (fpc_image_nhwc4), the forward on k_stem7x7 (fpc_conv2d code 3000; a row that does
not divide into 64-pixel segments: the implicit-GEMM kernel's generic loader), the weight gradient on k_stem_wgrad
(csrc/stem_train.hip) — and the 3x3 / stride-2 max-pool behind it is _MaxPoolFn (k_maxpool3x3s2 / k_maxpool3x3s2_bwd), counted
in stem_fwd_native / stem_wgrad_native / pool_fwd_native / pool_bwd_native: no convolution of the step is MIOpen's then.
The squeeze-and-excitation gate of the SE-ResNet blocks, the residual add and the ReLU behind it are torch's own by default (SEModule's
pool, two 1x1 convolutions, sigmoid and multiply, then an add and a ReLU); with FPC_TRAIN_NATIVE_SE=1 they are _SEGateAddReLUFn: the
forward on k_se_pool / k_se_excite / k_se_scale_add_relu (csrc/se.hip), the whole backward on csrc/se_train.hip, counted in
se_fwd_native / se_bwd_native (a refused block in se_torch).
The DEPTHWISE 3x3 convolution of the MobileNetV2 blocks and the ReLU6 behind their BatchNorms are torch's own by default (the grouped
MIOpen / aten kernels forward and both gradients, aten's hardtanh each way); with FPC_TRAIN_NATIVE_MBV2=1 the convolution is
_DepthwiseConv2dFn — the forward on the inference kernel k_dw_fwd (act 0, scale 1, shift 0), the data and weight gradients
beside it in csrc/depthwise.hip, counted in dw_fwd_native / dw_dgrad_native / dw_wgrad_native — and, with FPC_TRAIN_NATIVE_BN=1 as well,
ConvBNReLU6's BatchNorm and ReLU6 are one native op each way (batchnorm_act(relu6=True), counted in bn_relu6_native beside bn_native).
features.0 of the VGG encoders (3 -> 64 channels at full resolution, with a bias) and their five MaxPool2d(2, 2) are torch's own by
default (MIOpen forward and weight gradient, an aten reduction for the bias gradient, aten's pool with its int64 index plane and
scatter); with FPC_TRAIN_NATIVE_VGG=1 the convolution is _VggConv0Fn — fpc_image_nhwc4 and the inference kernel k_conv3x3_c3 (shift =
the bias, no activation) forward, k_c3_wgrad backward: the weight and the bias gradient from one pass over dy — and a pool is
_MaxPool2x2Fn (k_maxpool2x2 / k_maxpool2x2_bwd, the arg-max recomputed from x; csrc/vgg_train.hip), counted in c3_fwd_native /
c3_wgrad_native / pool2_fwd_native / pool2_bwd_native: no MIOpen convolution and no aten pooling kernel is left in a VGG step then.

The tiling / Winograd form of a shape is chosen once, by timing the candidates on the first call with that shape (this
synchronises: it happens in the warm-up steps).  f32 operands, accumulation and results, products in plain f32 or as the
exact bf16 x 3 split (FPC_SPLIT_PRECISION, default on), like the inference path.
`ENABLED = False` (or FPC_TRAIN_NATIVE_CONV=0) returns every convolution to torch's own kernels.
"""
import os

import torch

from fastposecnn_amd import _native as nat

ENABLED = bool(int(os.environ.get("FPC_TRAIN_NATIVE_CONV", "1")))
SPLIT_PRECISION = bool(int(os.environ.get("FPC_SPLIT_PRECISION", "1")))      # the bf16 x 3 product forms may be chosen
SPLIT_F16 = SPLIT_PRECISION and bool(int(os.environ.get("FPC_SPLIT_F16", "1")))      # ... and, for forward convolutions, the fp16 x 2 Winograd form
_plan_cache = {}            # (device index, B, Cin, H, W, Cout, k, stride, pad) -> nsplit code of fpc_conv2d
counters = {"fwd_native": 0, "dgrad_native": 0, "wgrad_native": 0, "dgrad_aten": 0, "wgrad_aten": 0, "wgrad_direct": 0,
            "grouped_fwd_native": 0, "grouped_dgrad_native": 0, "grouped_wgrad_native": 0,
            "stem_fwd_native": 0, "stem_wgrad_native": 0, "pool_fwd_native": 0, "pool_bwd_native": 0,
            "bn_native": 0, "bn_torch": 0, "se_fwd_native": 0, "se_bwd_native": 0, "se_torch": 0,
            "dw_fwd_native": 0, "dw_dgrad_native": 0, "dw_wgrad_native": 0, "bn_relu6_native": 0,
            "c3_fwd_native": 0, "c3_wgrad_native": 0, "pool2_fwd_native": 0, "pool2_bwd_native": 0}


# Weight-gradient sinks (round 6): an optimiser that keeps `p.grad` as views of one flat buffer (train_parallel.py) registers
# {weight data pointer -> GradSink}; the weight-gradient kernel then writes STRAIGHT into that view and the autograd function returns
# None for the weight — no temporary, no AccumulateGrad add launch per convolution (~70 of the ~270 add launches of a step), the
# sink's callback stands in for the post-accumulate hook.  A weight used twice in a step falls back to the ordinary path (the
# second gradient is returned and accumulated by autograd).
class GradSink:
    __slots__ = ("view", "callback", "written", "owner")

    def __init__(self, view, callback, owner):
        import weakref
        self.view, self.callback, self.written, self.owner = view, callback, False, weakref.ref(owner)


grad_sinks = {}


def _take_sink(w, aligned, padded=False):
    """The registered sink the weight-gradient kernel may write dW of `w` into, or None: no entry, one already written this step, a
    view of another shape, not contiguous or (where the caller's kernel needs it: `aligned`) not 16-byte aligned, or a gradient
    taken for a zero-padded copy of the weight (`padded`).  The entry of a dead owner is deleted."""
    sink = None if padded else grad_sinks.get(w.data_ptr())
    if sink is not None and sink.owner() is None:        # its optimiser is gone: the address may belong to another tensor now
        del grad_sinks[w.data_ptr()]
        return None
    if sink is None or sink.written or sink.view.shape != w.shape or not sink.view.is_contiguous() or (aligned and sink.view.data_ptr() % 16):
        return None
    return sink


def _commit_sink(sink):
    """dW was written in place: nothing is left for autograd to accumulate, the caller returns None for the weight."""
    sink.written = True
    sink.callback()


def _is_nhwc(t):
    return t.stride(1) == 1 and t.is_contiguous(memory_format=torch.channels_last)


def _channels_last(t):
    return t if _is_nhwc(t) else t.contiguous(memory_format=torch.channels_last)


def _operand(t, aligned=False, nhwc=True):
    """An incoming gradient or an input as the kernels read it: channel-last (nhwc=False: contiguous), and a copy of a tensor that
    is not 16-byte aligned where the caller's kernels need that (`aligned`)."""
    t = _channels_last(t) if nhwc else t.contiguous()
    if aligned and t.data_ptr() % 16:
        t = t.clone(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    return t


# ---- the conditions the gates share: each gate below is a conjunction of these and its own terms ---------------------------------

def _f32_cuda_4d(x, any_device=False):
    """f32 CUDA 4-D tensor on the current device (the launches go to its stream); any_device: on whichever"""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and (any_device or x.device.index == torch.cuda.current_device())


def _dense_nhwc(t):
    return _is_nhwc(t) and t.data_ptr() % 16 == 0


def _f32_param(t, dev):
    """contiguous 16-byte-aligned f32 parameter on `dev`: the kernels read it as it stands"""
    return t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.data_ptr() % 16 == 0


def _run(x, w, bias, stride, pad, code, out, up=None):
    B, Cin, H, W = x.shape
    Cout, _, Kh, Kw = w.shape
    Ho, Wo = out.shape[2], out.shape[3]
    L = nat.lib()
    sb, sc, sh, sw = x.stride()
    ws = nat.workspace("train_conv", x.device, L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, Cin, Cout, Kh, Kw, 0, 0, code))
    # (the library resolves its zero page — a device global — for the CURRENT device: make that the tensor's)
    with torch.cuda.device(x.device):
        nat.check(L.fpc_conv2d(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), None, nat.ptr(bias), None, nat.ptr(up), out.data_ptr(), None,
                               B, H, W, Cin, Cout, Kh, Kw, stride, pad, 0, 0, 0, code, ws.data_ptr(), ws.numel(), nat.stream()),
                  "fpc_conv2d (training)")


def conv_nhwc(x, w, bias, stride, pad, up=None, allow_f16=False):
    """x [B,Cin,H,W] channel-last, w OIHW contiguous -> [B,Cout,Ho,Wo] channel-last, on the engine's kernels.
    up [B,Cout,Ho/2,Wo/2] channel-last contiguous: added nearest-x2 upsampled in the kernel's epilogue (the FPN top-down merge)."""
    B, Cin, H, W = x.shape
    Cout, _, Kh, Kw = w.shape
    Ho, Wo = (H + 2 * pad - Kh) // stride + 1, (W + 2 * pad - Kw) // stride + 1
    out = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    key = (x.device.index, B, Cin, H, W, Cout, Kh, stride, pad, bool(allow_f16))
    code = _plan_cache.get(key)
    if code is None:
        cands = [0] + ([1000] if SPLIT_PRECISION else [])      # heuristic tiling; the same with split-precision products
        if Kh == 3 and Kw == 3 and stride == 1 and pad == 1 and Cin % 8 == 0 and Cout % 64 == 0:
            cands += [-1, -2, -4]       # Winograd F(2x2,3x3): 4 waves, 8 waves, 8 waves all-DMA
            if SPLIT_PRECISION:
                cands.append(-5)        # 8 waves, split-precision products
                cands.append(-7)        # the same products as four waves of 512 registers, weights straight into registers (wino_w4.hip)
                if Cout % 128 == 0:
                    cands.append(-6)    # 128 output channels per workgroup (wino128.hip)
                if allow_f16 and SPLIT_F16:
                    cands.append(-8)    # two fp16 pieces per operand (wino_h2.hip): FORWARD convolutions only — their operand is an
                    #                     activation of ordinary scale; a data gradient's operand is dy, whose values are tiny
                    #                     (the three-product form, -9, measured on the batch-8 step: forward 10.3-10.5 ms against 8.6-9.3 — its
                    #                     entry stages three K-steps and sixteen weight fragments; not a candidate here)
        if SPLIT_PRECISION and Kh == 1 and Kw == 1 and stride == 1 and pad == 0 and Cin in (64, 128) and Cout % 32 == 0:
            cands += [2000 + p for p in (1, 2, 4) if (Cout // 32) % p == 0]      # pixel-resident lateral product (lateral.hip)
        best = (float("inf"), 0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for c in cands:
            _run(x, w, bias, stride, pad, c, out)
            ev[0].record()
            for _ in range(3):
                _run(x, w, bias, stride, pad, c, out)
            ev[1].record()
            ev[1].synchronize()
            best = min(best, (ev[0].elapsed_time(ev[1]), c))
        code = _plan_cache[key] = best[1]
    _run(x, w, bias, stride, pad, code, out, up)
    return out


def _native_forward_ok(x, w):
    return w.shape[1] % 32 == 0 and w.shape[2] == w.shape[3]


def _dgrad_stride2(gy, w, H, W, pad):
    """dx [B,Cin,H,W] of a stride-2 convolution (1x1 pad 0, or 3x3 pad 1; H, W even) from dy [B,Cout,H/2,W/2]:
    y[i] = sum_k x[2 i + k - pad] w[k]  =>  dx[2 a] = dy[a] w[1],  dx[2 a + 1] = dy[a] w[2] + dy[a + 1] w[0]  per axis (3x3), i.e.
    per output parity (ry, rx) a 2-tap correlation of dy (zero past its end) with taps g_even = (w[1], 0), g_odd = (w[2], w[0])."""
    B, Cout, Ho, Wo = gy.shape
    Cin, K = w.shape[1], w.shape[2]
    gx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=gy.device, memory_format=torch.channels_last)
    wt = w.transpose(0, 1)                                              # [Cin, Cout, K, K]: output channels of the dgrad first
    if K == 1:
        gx.zero_()
        gx[:, :, ::2, ::2] = conv_nhwc(gy, wt.contiguous(), None, 1, 0)
        return gx
    gyp = torch.nn.functional.pad(gy, (0, 1, 0, 1))                     # one zero row / column past the end (channel-last stays)
    gyp = _channels_last(gyp)
    taps = ((1, None), (2, 0))                                           # parity -> kernel index of tap t = 0, 1 (None: no tap)
    for ry in range(2):
        for rx in range(2):
            if ry == 0 and rx == 0:
                out = conv_nhwc(gy, wt[:, :, 1:2, 1:2].contiguous(), None, 1, 0)
            else:
                g = torch.zeros((Cin, Cout, 2, 2), dtype=torch.float32, device=gy.device)
                for ty, ky in enumerate(taps[ry]):
                    for tx, kx in enumerate(taps[rx]):
                        if ky is not None and kx is not None:
                            g[:, :, ty, tx] = wt[:, :, ky, kx]
                out = conv_nhwc(gyp, g, None, 1, 0)
            gx[:, :, ry::2, rx::2] = out
    return gx


def _conv_backward(x, w, gy, stride, pad, needs, has_bias):
    """(dx, dW, db) of a convolution whose forward ran on the native kernels; needs = (x, W, bias) wanted."""
    Cout, Cin, Kh, Kw = w.shape
    gy = _operand(gy)
    need_x, need_w = needs[0], needs[1]
    gx = gw = gb = None
    if has_bias and needs[2]:
        gb = gy.sum((0, 2, 3))
    # a width the kernels' tiles do not divide (the heads: 7, 18, 24 channels): zero-padded copies of dy and W — the extra
    # channels contribute nothing to dx and their rows of dW are dropped
    w_full = w
    if (need_x and Cout % 32 != 0) or (need_w and Cout % 4 != 0):
        Cp = (Cout + 31) // 32 * 32
        gyp = torch.empty((gy.shape[0], Cp, gy.shape[2], gy.shape[3]), dtype=torch.float32, device=gy.device, memory_format=torch.channels_last)
        gyp[:, Cout:] = 0.0
        gyp[:, :Cout] = gy
        wp = torch.zeros((Cp, Cin, Kh, Kw), dtype=torch.float32, device=w.device)
        wp[:Cout] = w
        gy, w = gyp, wp
    Cw = w.shape[0]
    s2_native = (stride == 2 and pad == (Kh - 1) // 2 and Kh in (1, 3) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0)
    aten_x = need_x and not ((stride == 1 and pad <= Kh - 1) or s2_native)
    aten_w = need_w and Cin % 64 != 0
    if need_x and not aten_x:
        if stride == 1:
            # dx = conv(dy, W'), W'[ci][co][kh][kw] = W[co][ci][K-1-kh][K-1-kw], padding K-1-pad
            w2 = w.flip(2, 3).transpose(0, 1).contiguous() if Kh > 1 else w.transpose(0, 1).contiguous()
            gx = conv_nhwc(gy, w2, None, 1, Kh - 1 - pad)
        else:
            gx = _dgrad_stride2(gy, w, x.shape[2], x.shape[3], pad)
        counters["dgrad_native"] += 1
    if need_w and not aten_w:
        L = nat.lib()
        B, _, H, W = x.shape
        Ho, Wo = gy.shape[2], gy.shape[3]
        sink = _take_sink(w, aligned=False, padded=Cw != Cout)      # (no alignment check at this site, as before)
        gw = sink.view if sink is not None else torch.empty_like(w)
        sb, sc, sh, sw = x.stride()
        ws = nat.workspace("train_wgrad", x.device, L.fpc_conv2d_wgrad_workspace_bytes(B, Ho, Wo, Cin, Cw, Kh, Kw))
        wgrad = L.fpc_conv2d_wgrad_split if SPLIT_PRECISION else L.fpc_conv2d_wgrad
        nat.check(wgrad(x.data_ptr(), sb, sh, sw, gy.data_ptr(), gw.data_ptr(), B, H, W, Cin, Cw, Kh, Kw, stride,
                        pad, ws.data_ptr(), ws.numel(), nat.stream()), "fpc_conv2d_wgrad")
        if Cw != Cout:
            gw = gw[:Cout].contiguous()
        counters["wgrad_native"] += 1
        if sink is not None:
            _commit_sink(sink)
            gw = None
            counters["wgrad_direct"] += 1       # (counted at this site alone, as before)
    if aten_x or aten_w:
        ax, aw, _ = torch.ops.aten.convolution_backward(gy[:, :Cout] if Cw != Cout else gy, x, w_full, None, [stride, stride], [pad, pad],
                                                        [1, 1], False, [0, 0], 1, [aten_x, aten_w, False])
        if aten_x:
            gx = ax; counters["dgrad_aten"] += 1
        if aten_w:
            gw = aw; counters["wgrad_aten"] += 1
    return gx, gw, gb


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad):
        x = _channels_last(x)
        w = w.contiguous()
        ctx.stride, ctx.pad, ctx.has_bias = stride, pad, bias is not None
        ctx.save_for_backward(x, w)
        counters["fwd_native"] += 1
        return conv_nhwc(x, w, bias, stride, pad, allow_f16=True)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx, gw, gb = _conv_backward(x, w, gy, ctx.stride, ctx.pad, ctx.needs_input_grad, ctx.has_bias)
        return gx, gw, gb, None, None


class _ConvUpAddFn(torch.autograd.Function):
    """conv(x, w, bias) + nearest_x2(top): the FPN block's lateral 1x1 convolution and top-down merge
    (smp FPNBlock: F.interpolate(top, scale_factor=2, mode="nearest") + skip_conv(skip)) as ONE native launch — the
    engine's convolution epilogue adds the upsampled pyramid level, as on the inference path.  Backward: the convolution's
    as _Conv2dFn; the gradient of `top` is the 2 x 2 block sum of the output gradient."""

    @staticmethod
    def forward(ctx, x, w, bias, top, pad):
        x = _channels_last(x)
        w = w.contiguous()
        top = _channels_last(top)
        ctx.pad, ctx.has_bias = pad, bias is not None
        ctx.save_for_backward(x, w)
        counters["fwd_native"] += 1
        return conv_nhwc(x, w, bias, 1, pad, up=top)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _operand(gy)
        gx, gw, gb = _conv_backward(x, w, gy, 1, ctx.pad, ctx.needs_input_grad, ctx.has_bias)
        gt = torch.nn.functional.avg_pool2d(gy, 2, divisor_override=1) if ctx.needs_input_grad[3] else None
        return gx, gw, gb, gt, None


def conv2d_up_add(x, w, bias, top, pad):
    """conv(x) + nearest-x2(top) for the FPN merge; None when the shapes do not fit the fused form (the caller keeps the
    separate ops)."""
    if not (ENABLED and x.is_cuda and x.dtype == torch.float32 and top.dtype == torch.float32 and _native_forward_ok(x, w)):
        return None
    Cout = w.shape[0]
    Ho, Wo = x.shape[2] + 2 * pad - w.shape[2] + 1, x.shape[3] + 2 * pad - w.shape[3] + 1
    if Cout % 4 != 0 or Ho % 2 or Wo % 2 or tuple(top.shape) != (x.shape[0], Cout, Ho // 2, Wo // 2):
        return None
    return _ConvUpAddFn.apply(x, w, bias, top, int(pad))


# ---- the grouped 3x3 convolution (conv2 of the ResNeXt blocks) ---------------------------------------------------------------

# Off by default: with it off a grouped convolution is torch's own, forward and backward, as before (DESIGN.md 4.2a'').
NATIVE_GROUPED = bool(int(os.environ.get("FPC_TRAIN_NATIVE_GROUPED", "0")))
GROUPED_CG = (4, 8, 16, 32, 64)      # channels per group csrc/conv_grouped.hip is built for


def _grouped_native_op(op, cg, stride):
    """Whether `op` ("dgrad" / "wgrad") of the (channels per group, stride) combination runs native.  A combination whose native
    kernel measured slower than torch's on the training shapes is listed here and keeps torch's kernel (DESIGN.md 4.2a'', the
    per-site table); the forward always runs native."""
    return (op, cg, stride) not in _GROUPED_KEEP_TORCH


_GROUPED_KEEP_TORCH = frozenset()


def _grouped_ok(x, w, bias, stride, pad, groups):
    if not (ENABLED and NATIVE_GROUPED and torch.is_tensor(x) and _f32_cuda_4d(x) and w.dtype == torch.float32 and w.device == x.device):
        return False
    C = x.shape[1]
    # the bias is the kernel's `shift`, read as it stands: one value per channel
    if bias is not None and not (_f32_param(bias, x.device) and tuple(bias.shape) == (C,)):
        return False
    return (groups >= 1 and C % 32 == 0 and C % groups == 0 and C // groups in GROUPED_CG and tuple(w.shape) == (C, C // groups, 3, 3)
            and pad == 1 and stride in (1, 2) and x.numel() > 0)


class _GroupedConv2dFn(torch.autograd.Function):
    """The grouped 3x3 / pad-1 convolution on the native kernels, forward (k_conv3x3_grouped through fpc_conv2d_grouped, the bias as
    its shift) and backward (fpc_conv2d_grouped_dgrad / _wgrad, csrc/conv_grouped_train.hip).  One form: nothing is tuned."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, groups):
        x = _operand(x, aligned=True)
        w = w.contiguous()
        B, C, H, W = x.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        L = nat.lib()
        shift = None if bias is None else bias.detach()
        sb, sc, sh, sw = x.stride()
        ws = nat.workspace("train_grouped", x.device, L.fpc_conv2d_grouped_workspace_bytes(C, groups))
        nat.check(L.fpc_conv2d_grouped(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), None, nat.ptr(shift), out.data_ptr(), B, H, W, C,
                                       groups, stride, 0, 0, ws.data_ptr(), ws.numel(), nat.stream()), "fpc_conv2d_grouped (training)")
        ctx.stride, ctx.groups, ctx.has_bias = stride, groups, bias is not None
        ctx.save_for_backward(x, w)
        counters["grouped_fwd_native"] += 1
        return out

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, groups = ctx.stride, ctx.groups
        B, C, H, W = x.shape
        cg = C // groups
        gy = _operand(gy, aligned=True)
        Ho, Wo = gy.shape[2], gy.shape[3]
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx = gw = gb = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum((0, 2, 3))
        L = nat.lib()
        aten_x = need_x and not _grouped_native_op("dgrad", cg, stride)
        aten_w = need_w and not _grouped_native_op("wgrad", cg, stride)
        if need_x and not aten_x:
            gx = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            ws = nat.workspace("train_grouped", x.device, L.fpc_conv2d_grouped_dgrad_workspace_bytes(C, groups))
            nat.check(L.fpc_conv2d_grouped_dgrad(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), B, H, W, C, groups, stride, ws.data_ptr(),
                                                 ws.numel(), nat.stream()), "fpc_conv2d_grouped_dgrad")
            counters["grouped_dgrad_native"] += 1
        if need_w and not aten_w:
            sink = _take_sink(w, aligned=True)
            gw = sink.view if sink is not None else torch.empty_like(w)
            sb, sc, sh, sw = x.stride()
            ws = nat.workspace("train_grouped_wgrad", x.device, L.fpc_conv2d_grouped_wgrad_workspace_bytes(B, Ho, Wo, C, groups))
            nat.check(L.fpc_conv2d_grouped_wgrad(x.data_ptr(), sb, sh, sw, gy.data_ptr(), gw.data_ptr(), B, H, W, C, groups, stride,
                                                 ws.data_ptr(), ws.numel(), nat.stream()), "fpc_conv2d_grouped_wgrad")
            counters["grouped_wgrad_native"] += 1
            if sink is not None:
                _commit_sink(sink)
                gw = None
        if aten_x or aten_w:
            ax, aw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], groups,
                                                            [aten_x, aten_w, False])
            gx = ax if aten_x else gx
            gw = aw if aten_w else gw
        return gx, gw, gb, None, None


# ---- the depthwise 3x3 convolution (the MobileNetV2 blocks) -------------------------------------------------------------------

# Off by default: with it off a depthwise convolution is torch's own, forward and backward, and ReLU6 is never fused into the
# native BatchNorm, as before (DESIGN.md 4.2a''''''').
NATIVE_MBV2 = bool(int(os.environ.get("FPC_TRAIN_NATIVE_MBV2", "0")))
_DW_WALK_LIMIT = 2 ** 32 - 4096 * 256 - 8      # channel quads of a tensor: csrc/common.hpp's kWalkLimit


def _dw_native_op(op, stride):
    """Whether `op` ("dgrad" / "wgrad") of a depthwise convolution of this stride runs native.  A combination whose native kernel
    measured slower than torch's on the training shapes is listed here and keeps torch's kernel (DESIGN.md 4.2a''''''', the
    per-site table); the forward always runs native."""
    return (op, stride) not in _DW_KEEP_TORCH


_DW_KEEP_TORCH = frozenset()
_dw_identity = {}      # device index -> (ones, zeros): the forward kernel's scale / shift, grow-only


def _dw_scale_shift(dev, C):
    have = _dw_identity.get(dev.index)
    if have is None or have[0].numel() < C:
        have = _dw_identity[dev.index] = (torch.ones(C, dtype=torch.float32, device=dev), torch.zeros(C, dtype=torch.float32, device=dev))
    return have


def _depthwise_ok(x, w, bias, stride, pad, groups):
    return (ENABLED and NATIVE_MBV2 and torch.is_tensor(x) and _f32_cuda_4d(x) and torch.is_grad_enabled()
            and w.dtype == torch.float32 and w.device == x.device
            and groups == x.shape[1] and tuple(w.shape) == (x.shape[1], 1, 3, 3) and x.shape[1] % 4 == 0 and pad == 1
            and stride in (1, 2) and bias is None and 0 < x.numel() // 4 < _DW_WALK_LIMIT)


class _DepthwiseConv2dFn(torch.autograd.Function):
    """The depthwise 3x3 / pad-1 convolution without bias on the native kernels: forward k_dw_fwd through fpc_dwconv3x3 with the
    identity scale / shift and no activation, backward fpc_dwconv3x3_dgrad / _wgrad (csrc/depthwise.hip).  One form: nothing is tuned."""

    @staticmethod
    def forward(ctx, x, w, stride):
        x = _operand(x, aligned=True)
        w = _operand(w, aligned=True, nhwc=False)
        B, C, H, W = x.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        ones, zeros = _dw_scale_shift(x.device, C)
        nat.check(nat.lib().fpc_dwconv3x3(x.data_ptr(), w.data_ptr(), ones.data_ptr(), zeros.data_ptr(), out.data_ptr(), B, H, W, C, stride,
                                          0, nat.stream()), "fpc_dwconv3x3 (training)")
        ctx.stride = stride
        ctx.save_for_backward(x, w)
        counters["dw_fwd_native"] += 1
        return out

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride = ctx.stride
        B, C, H, W = x.shape
        gy = _operand(gy, aligned=True)
        Ho, Wo = gy.shape[2], gy.shape[3]
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx = gw = None
        L = nat.lib()
        aten_x = need_x and not _dw_native_op("dgrad", stride)
        aten_w = need_w and not _dw_native_op("wgrad", stride)
        if need_x and not aten_x:
            gx = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            nat.check(L.fpc_dwconv3x3_dgrad(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), B, H, W, C, stride, nat.stream()),
                      "fpc_dwconv3x3_dgrad")
            counters["dw_dgrad_native"] += 1
        if need_w and not aten_w:
            sink = _take_sink(w, aligned=True)
            gw = sink.view if sink is not None else torch.empty_like(w)
            ws = nat.workspace("train_dw_wgrad", x.device, L.fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C))
            nat.check(L.fpc_dwconv3x3_wgrad(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), B, H, W, C, stride, ws.data_ptr(), ws.numel(),
                                            nat.stream()), "fpc_dwconv3x3_wgrad")
            counters["dw_wgrad_native"] += 1
            if sink is not None:
                _commit_sink(sink)
                gw = None
        if aten_x or aten_w:
            ax, aw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], C,
                                                            [aten_x, aten_w, False])
            gx = ax if aten_x else gx
            gw = aw if aten_w else gw
        return gx, gw, None


# ---- the 7x7 / stride-2 stem (Cin = 3) and the 3x3 / stride-2 max-pool behind it -------------------------------------------

# Off by default: with it off the stem and the max-pool are torch's own, forward and backward, as before (DESIGN.md 4.2a''').
NATIVE_STEM = bool(int(os.environ.get("FPC_TRAIN_NATIVE_STEM", "0")))


def _stem_ok(x, w, bias, stride, pad):
    return (NATIVE_STEM and ENABLED and torch.is_tensor(x) and _f32_cuda_4d(x) and w.dtype == torch.float32 and w.device == x.device
            and tuple(w.shape) == (64, 3, 7, 7) and stride == 2 and pad == 3 and bias is None and x.shape[1] == 3
            and x.shape[0] >= 1 and x.shape[2] >= 8 and x.shape[3] >= 8 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
            and x.numel() < 2 ** 31
            and not x.requires_grad             # there is no data gradient here: an input that needs one stays on torch
            and torch.is_grad_enabled() and w.requires_grad)


class _StemConvFn(torch.autograd.Function):
    """The encoder's conv1 on the native kernels: y = conv(x, w) raw (training-mode BatchNorm follows), channel-last.  The NHWC4
    image is saved for the backward, which is the weight gradient alone (fpc_stem_wgrad): x gets no gradient."""

    @staticmethod
    def forward(ctx, x, w):
        x = _operand(x, aligned=True, nhwc=False)      # the planar image
        w = w.contiguous()
        B, _, H, W = x.shape
        Ho, Wo = H // 2, W // 2
        L = nat.lib()
        img4 = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device)
        nat.check(L.fpc_image_nhwc4(x.data_ptr(), img4.data_ptr(), B, H, W, nat.stream()), "fpc_image_nhwc4")
        out = torch.empty((B, 64, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        if Wo % 64 == 0:        # k_stem7x7: weights [64][4][7][7] (the image's fourth channel: zero weights), no scale / shift / ReLU
            w4 = torch.zeros((64, 4, 7, 7), dtype=torch.float32, device=x.device)
            w4[:, :3] = w.detach()
            ws = nat.workspace("train_conv", x.device, L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, 4, 64, 7, 7, 0, 0, 3000))
            nat.check(L.fpc_conv2d(img4.data_ptr(), 4 * H * W, 4 * W, 4, 1, w4.data_ptr(), None, None, None, None, out.data_ptr(), None,
                                   B, H, W, 4, 64, 7, 7, 2, 3, 0, 0, 0, 3000, ws.data_ptr(), ws.numel(), nat.stream()),
                      "fpc_conv2d (training, stem)")
        else:                   # a row k_stem7x7's 64-pixel segments do not divide: k_conv_igemm's generic loader on the NCHW image
            _run(x, w.detach(), None, 2, 3, 0, out)
        ctx.save_for_backward(img4, w)
        counters["stem_fwd_native"] += 1
        return out

    @staticmethod
    def backward(ctx, gy):
        img4, w = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None
        B, H, W, _ = img4.shape
        gy = _operand(gy, aligned=True)
        L = nat.lib()
        sink = _take_sink(w, aligned=True)
        gw = sink.view if sink is not None else torch.empty((64, 3, 7, 7), dtype=torch.float32, device=gy.device)
        ws = nat.workspace("train_stem_wgrad", gy.device, L.fpc_stem_wgrad_workspace_bytes(B, H, W))
        nat.check(L.fpc_stem_wgrad(img4.data_ptr(), gy.data_ptr(), gw.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), nat.stream()),
                  "fpc_stem_wgrad")
        counters["stem_wgrad_native"] += 1
        if sink is not None:
            _commit_sink(sink)
            gw = None
        return None, gw


class _MaxPoolFn(torch.autograd.Function):
    """max_pool2d(x, 3, 2, 1) on a dense channel-last tensor.  Only x is saved: the backward finds each window's arg-max again,
    by torch's rule (the first maximum in row-major order), and gathers dy (csrc/stem_train.hip: k_maxpool3x3s2_bwd)."""

    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        nat.check(nat.lib().fpc_maxpool3x3s2_fwd(x.data_ptr(), y.data_ptr(), B, H, W, C, nat.stream()), "fpc_maxpool3x3s2_fwd")
        ctx.save_for_backward(x)
        counters["pool_fwd_native"] += 1
        return y

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = _operand(gy, aligned=True)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        nat.check(nat.lib().fpc_maxpool3x3s2_bwd(x.data_ptr(), gy.data_ptr(), dx.data_ptr(), B, H, W, C, nat.stream()),
                  "fpc_maxpool3x3s2_bwd")
        counters["pool_bwd_native"] += 1
        return dx


def maxpool3x3s2(x):
    """max_pool2d(x, 3, 2, 1) on the native kernels, forward and backward, for a dense channel-last f32 GPU tensor that requires
    grad under autograd, with NATIVE_STEM set; None otherwise (the caller keeps torch's module)."""
    if not (NATIVE_STEM and ENABLED and torch.is_tensor(x) and _f32_cuda_4d(x) and torch.is_grad_enabled() and x.requires_grad
            and x.shape[1] % 4 == 0 and 0 < x.numel() < 2 ** 32 and _dense_nhwc(x)):
        return None
    return _MaxPoolFn.apply(x)


# ---- features.0 of the VGG encoders (3 -> 64 channels, 3x3 / stride 1 / pad 1) and their 2x2 / stride-2 max-pools ------------------

# Off by default: with it off features.0 and the pools are torch's own, forward and backward, as before (DESIGN.md 4.2a'''''''''''').
NATIVE_VGG = bool(int(os.environ.get("FPC_TRAIN_NATIVE_VGG", "0")))
_C3_WALK_LIMIT = 2 ** 32 - 4096 * 256 - 8      # csrc/common.hpp's kWalkLimit: 16 B H W below it (csrc/vgg.hip: conv3x3_c3_ok)
_c3_zero_shift = {}      # device index -> zeros [64]: the forward kernel's shift for a convolution without bias


def _vgg_c3_ok(x, w, bias, stride, pad, groups=1):
    return (NATIVE_VGG and ENABLED and torch.is_tensor(x) and _f32_cuda_4d(x) and w.dtype == torch.float32 and w.device == x.device
            and tuple(w.shape) == (64, 3, 3, 3) and stride == 1 and pad == 1 and groups == 1 and x.shape[1] == 3
            and (bias is None or (_f32_param(bias, x.device) and tuple(bias.shape) == (64,)))
            and x.shape[0] >= 1 and x.shape[2] >= 1 and x.shape[3] >= 1 and 16 * x.shape[0] * x.shape[2] * x.shape[3] < _C3_WALK_LIMIT
            and not x.requires_grad             # there is no data gradient here: an input that needs one stays on torch
            and torch.is_grad_enabled() and (w.requires_grad or (bias is not None and bias.requires_grad)))


class _VggConv0Fn(torch.autograd.Function):
    """features.0 of a VGG encoder on the native kernels: y = conv(x, w) + bias raw (BatchNorm or ReLU follows), channel-last, on
    k_conv3x3_c3.  The NHWC4 image is saved for the backward, which is the weight and bias gradient from one pass over dy
    (fpc_conv3x3_c3_wgrad, csrc/vgg_train.hip): x gets no gradient."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x = _operand(x, aligned=True, nhwc=False)      # the planar image
        w = _operand(w, aligned=True, nhwc=False)
        B, _, H, W = x.shape
        L = nat.lib()
        img4 = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device)
        nat.check(L.fpc_image_nhwc4(x.data_ptr(), img4.data_ptr(), B, H, W, nat.stream()), "fpc_image_nhwc4")
        out = torch.empty((B, 64, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        if bias is None:
            shift = _c3_zero_shift.get(x.device.index)
            if shift is None:
                shift = _c3_zero_shift[x.device.index] = torch.zeros(64, dtype=torch.float32, device=x.device)
        else:
            shift = bias.detach()
        nat.check(L.fpc_conv3x3_c3(img4.data_ptr(), w.data_ptr(), None, shift.data_ptr(), out.data_ptr(), B, H, W, 64, 0, nat.stream()),
                  "fpc_conv3x3_c3 (training)")
        ctx.has_bias = bias is not None
        ctx.save_for_backward(img4, w)
        counters["c3_fwd_native"] += 1
        return out

    @staticmethod
    def backward(ctx, gy):
        img4, w = ctx.saved_tensors
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_w or need_b):
            return None, None, None
        B, H, W, _ = img4.shape
        gy = _operand(gy, aligned=True)
        L = nat.lib()
        sink = _take_sink(w, aligned=True) if need_w else None
        gw = sink.view if sink is not None else torch.empty((64, 3, 3, 3), dtype=torch.float32, device=gy.device)
        gb = torch.empty(64, dtype=torch.float32, device=gy.device) if need_b else None
        ws = nat.workspace("train_c3_wgrad", gy.device, L.fpc_conv3x3_c3_wgrad_workspace_bytes(B, H, W))
        nat.check(L.fpc_conv3x3_c3_wgrad(img4.data_ptr(), gy.data_ptr(), gw.data_ptr(), nat.ptr(gb), B, H, W, ws.data_ptr(), ws.numel(),
                                         nat.stream()), "fpc_conv3x3_c3_wgrad")
        counters["c3_wgrad_native"] += 1
        if sink is not None:
            _commit_sink(sink)
            gw = None
        return None, gw if need_w else None, gb


class _MaxPool2x2Fn(torch.autograd.Function):
    """max_pool2d(x, 2, 2) on a dense channel-last tensor (k_maxpool2x2).  Only x is saved — it is alive anyway: the ReLU / BatchNorm
    in front saved it as its output —; the backward finds each window's arg-max again, by torch's rule (the first maximum in row-major
    order), and writes dy or 0 to every element (csrc/vgg_train.hip: k_maxpool2x2_bwd).  No index plane."""

    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        y = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        nat.check(nat.lib().fpc_maxpool2x2_fwd(x.data_ptr(), y.data_ptr(), B, H, W, C, nat.stream()), "fpc_maxpool2x2_fwd (training)")
        ctx.save_for_backward(x)
        counters["pool2_fwd_native"] += 1
        return y

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = _operand(gy, aligned=True)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        nat.check(nat.lib().fpc_maxpool2x2_bwd(x.data_ptr(), gy.data_ptr(), dx.data_ptr(), B, H, W, C, nat.stream()), "fpc_maxpool2x2_bwd")
        counters["pool2_bwd_native"] += 1
        return dx


def maxpool2x2(x):
    """max_pool2d(x, 2, 2) on the native kernels, forward and backward, for a dense channel-last f32 GPU tensor with even H and W and
    C % 4 == 0 that requires grad under autograd, with NATIVE_VGG set; None otherwise (the caller keeps torch's module)."""
    if not (NATIVE_VGG and ENABLED and torch.is_tensor(x) and _f32_cuda_4d(x) and torch.is_grad_enabled() and x.requires_grad
            and x.shape[0] >= 1 and x.shape[1] >= 4 and x.shape[1] % 4 == 0 and x.shape[2] >= 2 and x.shape[3] >= 2
            and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and x.numel() // 16 < _C3_WALK_LIMIT and _dense_nhwc(x)):
        return None
    return _MaxPool2x2Fn.apply(x)


def conv2d(x, w, bias, stride, pad, groups=1):
    """Training-mode convolution: native when the shapes allow it, torch otherwise (same signature either way).  A grouped
    convolution (conv2 of the ResNeXt blocks) is torch's own on the channel-last tensor, forward and backward, and like the stem
    counted neither as native nor as aten in `counters` — unless NATIVE_GROUPED (FPC_TRAIN_NATIVE_GROUPED=1) is set and it is
    a 3x3 / pad-1 / stride-1 or -2 convolution of the class csrc/conv_grouped.hip takes: then _GroupedConv2dFn, counted in
    grouped_fwd_native / grouped_dgrad_native / grouped_wgrad_native.  The 7x7 stem likewise: torch's own unless NATIVE_STEM
    (FPC_TRAIN_NATIVE_STEM=1) is set and it is the 3 -> 64 / stride-2 / pad-3 convolution without bias of an even-sized image
    that needs no gradient: then _StemConvFn, counted in stem_fwd_native / stem_wgrad_native.  A DEPTHWISE 3x3 / pad-1 / stride-1 or
    -2 convolution without bias (groups = C, C % 4 == 0) under autograd is _DepthwiseConv2dFn when NATIVE_MBV2
    (FPC_TRAIN_NATIVE_MBV2=1) is set, counted in dw_fwd_native / dw_dgrad_native / dw_wgrad_native; it is asked first.  features.0 of
    a VGG encoder (3 -> 64 channels, 3x3 / stride 1 / pad 1, with or without a bias, of an image that needs no gradient) is torch's
    own unless NATIVE_VGG (FPC_TRAIN_NATIVE_VGG=1) is set: then _VggConv0Fn, counted in c3_fwd_native / c3_wgrad_native."""
    if groups == 1 and _stem_ok(x, w, bias, stride, pad):
        return _StemConvFn.apply(x, w)
    if groups == 1 and _vgg_c3_ok(x, w, bias, stride, pad):
        return _VggConv0Fn.apply(x, w, bias)
    if groups != 1 and _depthwise_ok(x, w, bias, stride, pad, groups):
        return _DepthwiseConv2dFn.apply(x, w, int(stride))
    if groups != 1 and _grouped_ok(x, w, bias, stride, pad, groups):
        return _GroupedConv2dFn.apply(x, w, bias, int(stride), int(groups))
    # (the dense path asks neither for four dimensions nor for the current device, as before)
    if groups == 1 and ENABLED and x.is_cuda and x.dtype == torch.float32 and _native_forward_ok(x, w):
        return _Conv2dFn.apply(x, w, bias, int(stride), int(pad))
    if ENABLED and x.is_cuda and x.dim() == 4:
        x = _channels_last(x)        # the stem, a grouped convolution: keeps the rest of the network channel-last
    return torch.nn.functional.conv2d(x, w, bias, stride, pad, 1, groups)


# ---- bilinear upsampling (align_corners = True): the x2 of the segmentation blocks, the x4 of the heads ----------------

class _UpBilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, out_nhwc):
        B, C, h, w = x.shape
        fmt = torch.channels_last if out_nhwc else torch.contiguous_format
        out = torch.empty((B, C, h * scale, w * scale), dtype=torch.float32, device=x.device, memory_format=fmt)
        sb, sc, sh, sw = x.stride()
        L = nat.lib()
        nat.check(L.fpc_upsample_bilinear_fwd(x.data_ptr(), sb, sc, sh, sw, out.data_ptr(), B, C, h, w, scale, int(out_nhwc), nat.stream()),
                  "fpc_upsample_bilinear_fwd")
        ctx.scale, ctx.shape = scale, (B, C, h, w)
        ctx.in_nhwc = C > 1 and _is_nhwc(x)
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, h, w = ctx.shape
        fmt = torch.channels_last if ctx.in_nhwc else torch.contiguous_format
        gx = torch.empty((B, C, h, w), dtype=torch.float32, device=g.device, memory_format=fmt)
        sb, sc, sh, sw = g.stride()
        L = nat.lib()
        ws = nat.workspace("train_up_bwd", g.device, 4 * L.fpc_upsample_bilinear_bwd_scratch_floats(B, C, h, w, ctx.scale))
        nat.check(L.fpc_upsample_bilinear_bwd(g.data_ptr(), sb, sc, sh, sw, gx.data_ptr(), ws.data_ptr(), B, C, h, w, ctx.scale,
                                              int(ctx.in_nhwc), nat.stream()), "fpc_upsample_bilinear_bwd")
        return gx, None, None


def upsample_bilinear(x, scale, out_nchw=False):
    """F.interpolate(x, scale_factor=scale, mode='bilinear', align_corners=True) on the native kernels (forward and backward)
    for f32 GPU tensors with scale 2 or 4; torch otherwise.  The result keeps x's memory format unless out_nchw (the heads:
    full-resolution logits in the layout the losses and the post-network kernels read)."""
    if ENABLED and _f32_cuda_4d(x, any_device=True) and scale in (2, 4) and x.shape[0] * x.shape[1] <= 65535:
        nhwc = (not out_nchw) and x.shape[1] > 1 and _is_nhwc(x)
        if any(s < 0 for s in x.stride()) or x.stride(1) == 0:
            x = x.contiguous()
        return _UpBilinearFn.apply(x, int(scale), bool(nhwc))
    return torch.nn.functional.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=True)


# ---- GroupNorm(32 groups of 4 channels) + ReLU on channel-last activations (the decoder's Conv3x3GNReLU blocks) -----------

class _GroupNormReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps):
        B, C, H, W = x.shape
        L = nat.lib()
        y = torch.empty_like(x, memory_format=torch.channels_last)
        stats = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
        part = torch.empty(L.fpc_groupnorm4_relu_scratch_floats(B, H * W, C), dtype=torch.float32, device=x.device)
        gamma, beta = gamma.contiguous(), beta.contiguous()
        nat.check(L.fpc_groupnorm4_relu_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), stats.data_ptr(), part.data_ptr(),
                                            B, H * W, C, groups, float(eps), nat.stream()), "fpc_groupnorm4_relu_fwd")
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.groups = groups
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, stats = ctx.saved_tensors
        B, C, H, W = x.shape
        L = nat.lib()
        gy = _operand(gy)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        chunks = L.fpc_groupnorm4_relu_scratch_floats(B, H * W, C) // (B * C * 2)
        part = torch.empty((B, chunks, C, 2), dtype=torch.float32, device=x.device)
        nat.check(L.fpc_groupnorm4_relu_bwd(x.data_ptr(), gy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(), dx.data_ptr(),
                                            part.data_ptr(), B, H * W, C, ctx.groups, nat.stream()), "fpc_groupnorm4_relu_bwd")
        sums = part.sum((0, 1))                      # [C, 2]: dbeta, dgamma
        return dx, sums[:, 1].contiguous(), sums[:, 0].contiguous(), None, None


def groupnorm_relu(x, gn):
    """relu(gn(x)) for a torch.nn.GroupNorm `gn`: native on channel-last f32 GPU tensors whose groups are 4 channels wide
    (the decoder: GroupNorm(32, 128)), torch otherwise."""
    C, G = gn.num_channels, gn.num_groups
    if (ENABLED and _f32_cuda_4d(x, any_device=True) and gn.affine and C == 4 * G and 256 % G == 0 and G <= 64
            and x.shape[0] <= 65535 and _is_nhwc(x)):      # (channel-last, with no alignment term, as before)
        return _GroupNormReLUFn.apply(x, gn.weight, gn.bias, G, gn.eps)
    return torch.relu(gn(x))


# ---- training-mode BatchNorm2d (+ residual add) (+ ReLU) on channel-last activations (the encoder's blocks) -----------------

# Off by default: on the batch-8 step the native path has fewer launches and less kernel time, but the step time did not move by
# more than the spread between repeated runs (profiles/train_bn_step_kernels.txt).
NATIVE_BN = bool(int(os.environ.get("FPC_TRAIN_NATIVE_BN", "0")))


class _BatchNormActFn(torch.autograd.Function):
    """y = act(bn(x) + res) over the batch statistics, act 0 none / 1 ReLU / 2 ReLU6 (csrc/batchnorm.hip).  running_mean /
    running_var are rewritten through their raw pointers: their version counters do not move (PoseRegressor.note_unversioned_write)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var, eps, momentum, act):
        B, C, H, W = x.shape
        P = B * H * W
        L = nat.lib()
        y = torch.empty_like(x, memory_format=torch.channels_last)
        stats = torch.empty((C, 2), dtype=torch.float32, device=x.device)
        part = nat.workspace("train_bn", x.device, 4 * L.fpc_batchnorm_scratch_floats(P, C))
        nat.check(L.fpc_batchnorm_act_fwd(x.data_ptr(), nat.ptr(res), gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(),
                                          running_var.data_ptr(), y.data_ptr(), stats.data_ptr(), part.data_ptr(), P, C, float(eps),
                                          float(momentum), act, nat.stream()), "fpc_batchnorm_act_fwd")
        ctx.save_for_backward(x, gamma, stats, *((y,) if act else ()))
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, stats = ctx.saved_tensors[:3]
        y = ctx.saved_tensors[3] if ctx.act else None
        B, C, H, W = x.shape
        P = B * H * W
        L = nat.lib()
        gy = _operand(gy, aligned=True)
        dx = torch.empty_like(x, memory_format=torch.channels_last) if ctx.needs_input_grad[0] else None
        dres = torch.empty_like(x, memory_format=torch.channels_last) if ctx.needs_input_grad[1] else None
        dgb = torch.empty((2, C), dtype=torch.float32, device=x.device)
        part = nat.workspace("train_bn", x.device, 4 * L.fpc_batchnorm_scratch_floats(P, C))
        nat.check(L.fpc_batchnorm_act_bwd(x.data_ptr(), nat.ptr(y), gy.data_ptr(), gamma.data_ptr(), stats.data_ptr(), nat.ptr(dx),
                                          nat.ptr(dres), dgb.data_ptr(), dgb.data_ptr() + 4 * C, part.data_ptr(), P, C, ctx.act,
                                          nat.stream()), "fpc_batchnorm_act_bwd")
        return (dx, dres, dgb[0] if ctx.needs_input_grad[2] else None, dgb[1] if ctx.needs_input_grad[3] else None,
                None, None, None, None, None)


def batchnorm_act(x, bn, res=None, relu=True, count_refusal=True, relu6=False):
    """relu(bn(x) + res) (res and relu optional; a residual needs relu; relu6=True: min(max(bn(x), 0), 6) in place of the ReLU, with
    no residual — a MobileNetV2 block has none there —, counted in bn_relu6_native too) for a torch.nn.BatchNorm2d `bn` in TRAINING mode, as one
    native op each way on dense channel-last f32 GPU tensors: batch statistics, the module's running statistics and
    num_batches_tracked updated as torch does.  None when the native path does not apply — evaluation mode, no affine parameters,
    no running statistics, momentum=None (torch's cumulative average), another layout (never a layout copy to get here) or
    dtype, a tensor that is not on the current device, fewer than two values per channel, the switch FPC_TRAIN_NATIVE_BN off (its
    default) — and the caller runs the torch modules (counted as
    bn_torch unless the caller says it will ask again)."""
    ok = (ENABLED and NATIVE_BN and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None
          and bn.running_mean is not None and torch.is_tensor(x) and _f32_cuda_4d(x)
          and x.shape[1] % 4 == 0 and x.shape[1] == bn.num_features and 2 <= x.shape[0] * x.shape[2] * x.shape[3] < 2 ** 31 - 256
          and _dense_nhwc(x) and not (relu6 and res is not None)
          and (res is None or (relu and res.shape == x.shape and res.dtype == x.dtype and res.device == x.device and _dense_nhwc(res)))
          and all(_f32_param(t, x.device) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)))
    if not ok:
        counters["bn_torch"] += int(count_refusal)
        return None
    bn.num_batches_tracked.add_(1)
    counters["bn_native"] += 1
    counters["bn_relu6_native"] += int(bool(relu6))
    return _BatchNormActFn.apply(x, res, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                                 2 if relu6 else int(bool(relu)))


# ---- the squeeze-and-excitation gate + residual add + ReLU of the SE-ResNet blocks (behind bn3) ------------------------------

# Off by default: with it off the gate is SEModule's chain of torch ops, the add and the ReLU two more, forward and backward, as
# before (DESIGN.md 4.2a''''').
NATIVE_SE = bool(int(os.environ.get("FPC_TRAIN_NATIVE_SE", "0")))


class _SEGateAddReLUFn(torch.autograd.Function):
    """y = relu(x * sigmoid(fc2(relu(fc1(mean_hw(x))))) + res) on dense channel-last tensors: the forward on the inference kernels
    (csrc/se.hip; k_se_excite also writes the means and the hidden activations), the whole backward on csrc/se_train.hip.
    w1 [Cr, C, 1, 1] / w2 [C, Cr, 1, 1] are fc1's / fc2's weights as they stand; their gradients come back as views of those shapes."""

    @staticmethod
    def forward(ctx, x, res, w1, b1, w2, b2):
        B, C, H, W = x.shape
        Cr = w1.shape[0]
        L = nat.lib()
        dev = x.device
        gate = torch.empty((B, C), dtype=torch.float32, device=dev)
        mean = torch.empty((B, C), dtype=torch.float32, device=dev)
        hidden = torch.empty((B, Cr), dtype=torch.float32, device=dev)
        y = torch.empty_like(x, memory_format=torch.channels_last)
        ws = nat.workspace("train_se", dev, 4 * L.fpc_se_scratch_floats(B, H, W, C))
        nat.check(L.fpc_se_gate_train(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), gate.data_ptr(),
                                      mean.data_ptr(), hidden.data_ptr(), ws.data_ptr(), B, H, W, C, C // Cr, nat.stream()),
                  "fpc_se_gate_train")
        nat.check(L.fpc_se_scale_add_relu(x.data_ptr(), gate.data_ptr(), res.data_ptr(), y.data_ptr(), B, H, W, C, nat.stream()),
                  "fpc_se_scale_add_relu (training)")
        ctx.save_for_backward(x, y, gate, mean, hidden, w1, w2)
        counters["se_fwd_native"] += 1
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, gate, mean, hidden, w1, w2 = ctx.saved_tensors
        B, C, H, W = x.shape
        Cr = w1.shape[0]
        L = nat.lib()
        gy = _operand(gy, aligned=True)
        need = ctx.needs_input_grad
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        dres = torch.empty_like(x, memory_format=torch.channels_last) if need[1] else None
        # one buffer for the four parameter gradients: dw2 [C][Cr], dw1 [Cr][C], db2 [C], db1 [Cr] (every offset a multiple of 64 floats)
        flat = torch.empty(2 * C * Cr + C + Cr, dtype=torch.float32, device=x.device)
        dw2, dw1, db2, db1 = flat.split((C * Cr, C * Cr, C, Cr))
        ws = nat.workspace("train_se_bwd", x.device, 4 * L.fpc_se_bwd_scratch_floats(B, H, W, C, C // Cr))
        nat.check(L.fpc_se_bwd(x.data_ptr(), y.data_ptr(), gy.data_ptr(), gate.data_ptr(), mean.data_ptr(), hidden.data_ptr(),
                               w1.data_ptr(), w2.data_ptr(), dx.data_ptr(), nat.ptr(dres), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(),
                               db2.data_ptr(), ws.data_ptr(), B, H, W, C, C // Cr, nat.stream()), "fpc_se_bwd")
        counters["se_bwd_native"] += 1
        return (dx if need[0] else None, dres, dw1.view(w1.shape) if need[2] else None, db1 if need[3] else None,
                dw2.view(w2.shape) if need[4] else None, db2 if need[5] else None)


def _se_fc_ok(fc, cin, cout, dev):
    return (isinstance(fc, torch.nn.Conv2d) and fc.kernel_size == (1, 1) and fc.stride == (1, 1) and fc.padding == (0, 0)
            and fc.dilation == (1, 1) and fc.groups == 1 and fc.bias is not None and fc.in_channels == cin and fc.out_channels == cout
            and _f32_param(fc.weight, dev) and _f32_param(fc.bias, dev))


def se_gate_add_relu(x, se_module, res, act=None):
    """act(se_module(x) + res) of an SEResNetBottleneck — x is bn3's output, `act` the block's activation — as one native op each
    way (_SEGateAddReLUFn), with NATIVE_SE (FPC_TRAIN_NATIVE_SE=1) set, under autograd, for dense channel-last 16-byte-aligned f32
    tensors of one shape on the current device with C % 64 == 0 and C <= 8192, an se_module whose fc1 / fc2 are biased 1x1
    convolutions with contiguous aligned f32 parameters, and nn.ReLU as BOTH the block's activation (act=None: the caller's is a
    plain ReLU) and the gate's (a test may have swapped either for a smooth activation).  None otherwise — never a layout copy to get here — and the caller runs the
    torch modules (counted in se_torch)."""
    ok = (ENABLED and NATIVE_SE and torch.is_grad_enabled() and torch.is_tensor(x) and torch.is_tensor(res) and _f32_cuda_4d(x)
          and res.dtype == torch.float32 and res.device == x.device and res.shape == x.shape
          and x.shape[1] % 64 == 0 and 64 <= x.shape[1] <= 8192 and 1 <= x.shape[0] <= 65535 and x.shape[2] >= 1 and x.shape[3] >= 1
          and x.numel() // 4 < 2 ** 32 - 4096 * 256 - 8 and _dense_nhwc(x) and _dense_nhwc(res)
          and (act is None or isinstance(act, torch.nn.ReLU)) and isinstance(getattr(se_module, "relu", None), torch.nn.ReLU)
          and isinstance(getattr(se_module, "sigmoid", None), torch.nn.Sigmoid)
          and isinstance(getattr(se_module, "fc1", None), torch.nn.Conv2d) and se_module.fc1.out_channels >= 1
          and x.shape[1] % se_module.fc1.out_channels == 0
          and _se_fc_ok(se_module.fc1, x.shape[1], se_module.fc1.out_channels, x.device)
          and _se_fc_ok(getattr(se_module, "fc2", None), se_module.fc1.out_channels, x.shape[1], x.device))
    if not ok:
        counters["se_torch"] += 1
        return None
    fc1, fc2 = se_module.fc1, se_module.fc2
    return _SEGateAddReLUFn.apply(x, res, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
