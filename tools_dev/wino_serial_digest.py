"""SHA-256 of what the four-wave Winograd kernels (csrc/wino_tile.hpp: wino_w4.hip, wino_h2.hip, wino_h3.hip) write on a fixed list
of small launches: every output tensor and every GroupNorm record tensor, both pre-filled with NaN.  The set-up around the K loop
and the output transform may be rearranged, the arithmetic may not: the digests of a change there equal the committed ones
(tests/golden/wino_serial_digests.json, written by this script on the commit BEFORE the change; tests/test_gpu_wino_serial.py).
    python tools_dev/wino_serial_digest.py > tests/golden/wino_serial_digests.json
Operands are generated on the CPU from seeds.  The list: requests -7 .. -11 of fpc_conv2d; Cin 16 and 48 (32 too for the forms that
run pairs of K-steps); Cout 64 and 128; 24 x 32 and 23 x 31 at B = 2, 3, 5 (transposed launches with a seam in the middle patch and
a ragged last canvas row), 40 x 24 at B = 2, 3 (the orientation rule leaves it alone; it packs with a seam); epilogues none, folded
BatchNorm + residual + ReLU, GroupNorm records; and the folded s2.0 (four decoders as groups) at p2 = 24 x 32, B = 2, 3, in both
orientations, through the engine (every 3x3 site on form 9, no autotuning: the plans are the same on every build)."""
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

REQUESTS = (-7, -8, -9, -10, -11)
SHAPES = [(B, H, W) for H, W in ((24, 32), (23, 31)) for B in (2, 3, 5)] + [(2, 40, 24), (3, 40, 24)]
COUTS = (64, 128)
EPILOGUES = ("none", "bn_relu_res", "gn")
FOLD_B = (2, 3)
FOLD_HW = (96, 128)      # p2 = 24 x 32


def cins(request):
    return (16, 32, 48) if request <= -9 else (16, 48)


def conv_cases(request):
    """(name, request, B, Cin, H, W, Cout, epilogue) of one request, in a fixed order."""
    return [(f"r{request}-b{B}-{Cin}x{H}x{W}-{Cout}-{epi}", request, B, Cin, H, W, Cout, epi)
            for B, H, W in SHAPES for Cin in cins(request) for Cout in COUTS for epi in EPILOGUES]


@functools.lru_cache(maxsize=None)
def operands(B, Cin, H, W, Cout):
    """x [B,Cin,H,W], w [Cout,Cin,3,3], scale, shift [Cout], res [B,Cout,H,W] on the CPU; one set per shape, shared by every request and
    epilogue."""
    g = torch.Generator().manual_seed(((B * 64 + Cin) * 64 + H) * 256 + W * 2 + Cout // 128)
    x = torch.randn((B, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    res = torch.randn((B, Cout, H, W), generator=g)
    return x, w, scale, shift, res


def epilogue_args(epi, scale, shift, res):
    """What the epilogue `epi` takes of (scale, shift, res NCHW): (scale, shift, res, relu, gn)"""
    if epi == "bn_relu_res":
        return scale, shift, res, True, False
    return None, None, None, False, epi == "gn"


def run_conv(dev, request, x, w, scale=None, shift=None, res=None, relu=False, gn=False):
    """One fpc_conv2d launch on CPU operands (x, res NCHW): (out [B,H,W,Cout], records or None), on the CPU."""
    from test_gpu_wino_pack import _conv
    t = lambda a: None if a is None else a.contiguous().to(dev)
    out, gp, _ = _conv(dev, x.permute(0, 2, 3, 1).contiguous().to(dev), w.contiguous().to(dev), request, scale=t(scale), shift=t(shift),
                       res=None if res is None else res.permute(0, 2, 3, 1).contiguous().to(dev), relu=relu, gn=gn)
    return out.cpu(), None if gp is None else gp.cpu()


def run_case(dev, case):
    _, request, B, Cin, H, W, Cout, epi = case
    x, w, scale, shift, res = operands(B, Cin, H, W, Cout)
    s, h, r, relu, gn = epilogue_args(epi, scale, shift, res)
    return run_conv(dev, request, x, w, scale=s, shift=h, res=r, relu=relu, gn=gn)


def fold_engine(dev, B):
    """(model, engine) with every 3x3 / stride-1 site on form 9 and s2.0 folded, planned without timing anything."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd.engine import NetEngine
    from test_gpu_p2_fold import _model
    m, _ = _model(L)
    m = m.to(dev)
    eng = NetEngine(m, B, FOLD_HW[0], FOLD_HW[1], dev, autotune=False, split_precision=3)
    eng.force_winograd(9)
    eng.force_fold(1)
    assert any(p[2] == 5000 for p in eng.conv_plans()), "s2.0 is not folded"
    return m, eng


def run_fold(dev, B, orient, built=None):
    """{name: CPU tensor}: s2.0's output of the four decoders and the logits (which the GroupNorm records of s2.0 feed)."""
    from fastposecnn_amd import synth
    m, eng = built or fold_engine(dev, B)
    eng.set_wino_orient(orient)
    x = torch.stack([synth.make_image(i, *FOLD_HW) for i in range(B)]).to(dev)
    with torch.no_grad():
        logits, _ = eng.forward(x)
    torch.cuda.synchronize()
    out = {f"fold-b{B}-orient{orient}-d{d}.seg6": eng.tensor(f"d{d}.seg6").detach().cpu().clone() for d in range(4)}
    out.update({f"fold-b{B}-orient{orient}-logits.{k}": v.detach().cpu().clone() for k, v in sorted(logits.items())})
    return out


def digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def case_digests(dev, case):
    out, gp = run_case(dev, case)
    d = {case[0] + ":out": digest(out)}
    if gp is not None:
        d[case[0] + ":records"] = digest(gp)
    return d


def main():
    dev = torch.device("cuda:0")
    d = {}
    for request in REQUESTS:
        for case in conv_cases(request):
            d.update(case_digests(dev, case))
    for B in FOLD_B:
        built = fold_engine(dev, B)
        for orient in (1, 0):
            d.update({k: digest(v) for k, v in run_fold(dev, B, orient, built).items()})
    json.dump(d, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
