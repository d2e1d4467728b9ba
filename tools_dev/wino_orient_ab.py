"""Alternates request -9 (plain) and -11 (orientation rule) of fpc_conv2d on the headline's wide-map shapes at batch 32; run under
rocprofv3 --kernel-trace, parsed by wino_orient_ab_parse.py (the k_conv_wino_h3 dispatches in launch order)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fastposecnn_amd import _native as nat
SHAPES = [("layer1", 32, 64, 120, 160, 64), ("s2.0-unfolded", 32, 256, 120, 160, 128), ("layer2", 32, 128, 60, 80, 128), ("s3.0", 32, 256, 60, 80, 128)]
WARM, N = 3, 20
dev = torch.device("cuda:0")
L = nat.lib()
for name, B, Cin, H, W, Cout in SHAPES:
    x = torch.randn((B, H, W, Cin), device=dev)
    w = torch.randn((Cout, Cin, 3, 3), device=dev) * 0.05
    out = torch.empty((B, H, W, Cout), device=dev)
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, H, W, Cin, Cout, 3, 3), dtype=torch.uint8, device=dev)
    sb, sh, sw, sc = x.stride()
    st = torch.cuda.current_stream().cuda_stream
    for i in range(WARM + N):
        for ns in (-9, -11):
            nat.check(L.fpc_conv2d(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), None, None, None, None, out.data_ptr(), None, B, H, W, Cin,
                                   Cout, 3, 3, 1, 1, 0, 0, 0, ns, ws.data_ptr(), ws.numel(), st), "conv")
        torch.cuda.synchronize()
print("done")
