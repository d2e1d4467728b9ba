"""SHA-256 of what every entry of the depthwise family writes (csrc/depthwise.hip): fpc_dwconv3x3, fpc_dwconv3x3_dgrad / _wgrad (pad 1,
MobileNetV2) and fpc_mbconv_dw, fpc_mbconv_dw_dgrad / _wgrad (the static "same" pads, EfficientNet-B0), every output buffer pre-filled
with NaN (the weight gradient's workspace too), the operands drawn on the CPU from a seed the case alone fixes.  Written on the commit
BEFORE the two encoders' copies of these kernels became one family (tests/golden/depthwise_digests.json);
tests/test_gpu_depthwise_family.py compares the change against it.
    python tools_dev/depthwise_digest.py > tests/golden/depthwise_digests.json
The shapes (B, Hi, Wi, C), each for a way a merged kernel can go wrong: 2 x 2 (every tap pads somewhere), 6 x 10 (strip and block
tails), 3 x 30 x 40 x 144 (126 workgroups: the XCD-banded walk, several slices), 1152 channels (more than 256 channel quads),
2 x 22 x 80 x 8 (slice seams inside frames), 4 x 6 (fewer units than pixel slots); the pad-1 entries at stride 2 also take
2 x 21 x 79 x 8, whose odd extents walk the tail guards of their stride-2 data gradient.  The forward runs with a non-trivial scale
and shift at every activation code the entry knows.  The pad-1 entries at stride 1 and the "same" entries at (3, 1) get the same
operands: they are one convolution."""
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

SHAPES = [(2, 2, 2, 4), (1, 6, 10, 32), (3, 30, 40, 144), (1, 16, 4, 1152), (2, 22, 80, 8), (1, 4, 6, 8)]
ODD = (2, 21, 79, 8)                                  # pad-1 entries, stride 2 only
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]                 # (k, stride) of the "same" entries
OPS = ("fwd", "dgrad", "wgrad")


def cases():
    """(name, family, op, shape, k, stride, act) in a fixed order; family "dw3" is the pad-1 entries, "mb" the "same"-pad ones"""
    out = []
    for op in OPS:
        for s in (1, 2):
            for shape in SHAPES + ([ODD] if s == 2 else []):
                for act in ((0, 1) if op == "fwd" else (0,)):
                    out.append(("dw3-%s-s%d-B%d-%dx%d-C%d-act%d" % ((op, s) + shape + (act,)), "dw3", op, shape, 3, s, act))
        for k, s in KS:
            for shape in SHAPES:
                for act in ((0, 1, 2) if op == "fwd" else (0,)):
                    out.append(("mb-%s-k%ds%d-B%d-%dx%d-C%d-act%d" % ((op, k, s) + shape + (act,)), "mb", op, shape, k, s, act))
    return out


def out_hw(family, Hi, Wi, stride):
    return ((Hi - 1) // stride + 1, (Wi - 1) // stride + 1) if family == "dw3" else (Hi // stride, Wi // stride)


@functools.lru_cache(maxsize=None)
def operands(shape, k, stride, ceil):
    """x [B,Hi,Wi,C], w [C,1,k,k], scale, shift [C], dy [B,Ho,Wo,C] on the CPU; ceil: the pad-1 output extents.  One set per
    (shape, k, stride), shared by both families where their output extents agree, by the three operations and every activation."""
    B, Hi, Wi, C = shape
    Ho, Wo = out_hw("dw3" if ceil else "mb", Hi, Wi, stride)
    g = torch.Generator().manual_seed((((B * 128 + Hi) * 128 + Wi) * 2048 + C) * 16 + 4 * k + stride)
    x = torch.randn((B, Hi, Wi, C), generator=g)
    w = torch.randn((C, 1, k, k), generator=g) / k
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    dy = torch.randn((B, Ho, Wo, C), generator=g)
    return x, w, scale, shift, dy


def run_case(dev, case):
    """the entry's output on the CPU, flat; unwritten elements stay NaN"""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    _, family, op, shape, k, s, act = case
    B, Hi, Wi, C = shape
    Ho, Wo = out_hw(family, Hi, Wi, s)
    x, w, scale, shift, dy = (t.to(dev) for t in operands(shape, k, s, (Ho, Wo) != (Hi // s, Wi // s)))
    mb = family == "mb"
    ks = (k, s) if mb else (s,)
    n = {"fwd": B * Ho * Wo * C, "dgrad": B * Hi * Wi * C, "wgrad": C * k * k}[op]
    out = torch.full((n,), float("nan"), device=dev)
    if op == "fwd":
        fn = L.fpc_mbconv_dw if mb else L.fpc_dwconv3x3
        rc = fn(x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), B, Hi, Wi, C, *ks, act, nat.stream())
    elif op == "dgrad":
        fn = L.fpc_mbconv_dw_dgrad if mb else L.fpc_dwconv3x3_dgrad
        rc = fn(dy.data_ptr(), w.data_ptr(), out.data_ptr(), B, Hi, Wi, C, *ks, nat.stream())
    else:
        need = L.fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, k) if mb else L.fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C)
        ws = torch.full((need // 4 + 64,), float("nan"), device=dev)
        fn = L.fpc_mbconv_dw_wgrad if mb else L.fpc_dwconv3x3_wgrad
        rc = fn(x.data_ptr(), dy.data_ptr(), out.data_ptr(), B, Hi, Wi, C, *ks, ws.data_ptr(), need, nat.stream())
    assert rc == 0, (case[0], rc)
    torch.cuda.synchronize()
    return out.cpu()


def digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def main():
    dev = torch.device("cuda:0")
    d = {case[0]: digest(run_case(dev, case)) for case in cases()}
    json.dump(d, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
