"""SHA-256 of what k_conv_wino_h3 writes on the launches that walk its two exits (csrc/wino_tile.hpp: wino_output — the fast exit
of a workgroup whose patch lies wholly inside its frame, the general one of every other): every output tensor and every GroupNorm
record tensor, both pre-filled with NaN.  Written on the commit BEFORE the exits were parted (tests/golden/wino_exit_digests.json);
tests/test_gpu_wino_exit.py compares the change against it, as tests/test_gpu_wino_serial.py does on its own shapes.
    python tools_dev/wino_exit_digest.py > tests/golden/wino_exit_digests.json
The list: requests -9, -11, -12, -13 of fpc_conv2d; Cin 16; Cout 64 and 128; 16 x 16 and 32 x 32 (every patch inside), 18 x 16 and
16 x 18 (one partial row / column of patches), 20 x 16 (transposed under -11 and -13), 16 x 20 (ten tile columns: seams after 2, 4
and 6 at B = 5, after 2 at B = 3) and 16 x 22 (eleven: the row-split map), all at B = 3 — a ragged last canvas row, whose seam
patch has no second frame — and 16 x 20 at B = 5 too; epilogues none, folded BatchNorm + residual + ReLU, GroupNorm records; and the
folded s2.0 (four decoders as groups) at p2 = 24 x 32 and 32 x 32, B = 2, 3, in both orientations, through the engine."""
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

REQUESTS = (-9, -11, -12, -13)
GENERAL_EXIT = -100      # fpc.h: FPC_PLAN_WINO_GENERAL_EXIT + request = the request with every workgroup on the general exit
SHAPES = [(3, 16, 16), (3, 32, 32), (3, 18, 16), (3, 16, 18), (3, 20, 16), (3, 16, 20), (5, 16, 20), (3, 16, 22)]
CIN = 16
COUTS = (64, 128)
EPILOGUES = ("none", "bn_relu_res", "gn")
FOLD_B = (2, 3)
FOLD_HW = ((96, 128), (128, 128))      # p2 = 24 x 32 and 32 x 32


def conv_cases(request):
    """(name, request, B, Cin, H, W, Cout, epilogue) of one request, in a fixed order."""
    return [(f"r{request}-b{B}-{CIN}x{H}x{W}-{Cout}-{epi}", request, B, CIN, H, W, Cout, epi)
            for B, H, W in SHAPES for Cout in COUTS for epi in EPILOGUES]


@functools.lru_cache(maxsize=None)
def operands(B, Cin, H, W, Cout):
    """x [B,Cin,H,W], w [Cout,Cin,3,3], scale, shift [Cout], res [B,Cout,H,W] on the CPU; one set per shape, shared by every request and
    epilogue."""
    g = torch.Generator().manual_seed(((B * 64 + Cin) * 64 + H) * 256 + W * 2 + Cout // 128 + 77)
    x = torch.randn((B, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    res = torch.randn((B, Cout, H, W), generator=g)
    return x, w, scale, shift, res


def run_case(dev, case, general=False):
    """(out [B,H,W,Cout], records or None) on the CPU; general: every workgroup on the general exit"""
    from test_gpu_wino_pack import _conv
    _, request, B, Cin, H, W, Cout, epi = case
    x, w, scale, shift, res = operands(B, Cin, H, W, Cout)
    bn = epi == "bn_relu_res"
    t = lambda a: a.contiguous().to(dev) if bn else None
    out, gp, _ = _conv(dev, x.permute(0, 2, 3, 1).contiguous().to(dev), w.contiguous().to(dev), request + (GENERAL_EXIT if general else 0),
                       scale=t(scale), shift=t(shift), res=t(res.permute(0, 2, 3, 1)), relu=bn, gn=epi == "gn")
    return out.cpu(), None if gp is None else gp.cpu()


def fold_engine(dev, B, hw):
    """(model, engine) with every 3x3 / stride-1 site on form 9 and s2.0 folded, planned without timing anything."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd.engine import NetEngine
    from test_gpu_p2_fold import _model
    m, _ = _model(L)
    m = m.to(dev)
    eng = NetEngine(m, B, hw[0], hw[1], dev, autotune=False, split_precision=3)
    eng.force_winograd(9)
    eng.force_fold(1)
    assert any(p[2] == 5000 for p in eng.conv_plans()), "s2.0 is not folded"
    return m, eng


def run_fold(dev, B, hw, orient, built):
    """{name: CPU tensor}: s2.0's output of the four decoders and the logits (which the GroupNorm records of s2.0 feed)."""
    from fastposecnn_amd import synth
    m, eng = built
    eng.set_wino_orient(orient)
    x = torch.stack([synth.make_image(i, *hw) for i in range(B)]).to(dev)
    with torch.no_grad():
        logits, _ = eng.forward(x)
    torch.cuda.synchronize()
    tag = f"fold-{hw[0]}x{hw[1]}-b{B}-orient{orient}"
    out = {f"{tag}-d{d}.seg6": eng.tensor(f"d{d}.seg6").detach().cpu().clone() for d in range(4)}
    out.update({f"{tag}-logits.{k}": v.detach().cpu().clone() for k, v in sorted(logits.items())})
    return out


def digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def main():
    dev = torch.device("cuda:0")
    d = {}
    for request in REQUESTS:
        for case in conv_cases(request):
            out, gp = run_case(dev, case)
            d[case[0] + ":out"] = digest(out)
            if gp is not None:
                d[case[0] + ":records"] = digest(gp)
    for hw in FOLD_HW:
        for B in FOLD_B:
            built = fold_engine(dev, B, hw)
            for orient in (1, 0):
                d.update({k: digest(v) for k, v in run_fold(dev, B, hw, orient, built).items()})
    json.dump(d, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
