"""The training step's grouped 3x3 convolution (csrc/conv_grouped.hip, csrc/conv_grouped_train.hip) on the seven conv2 site shapes of
ResNeXt-50-32x4d at 640 x 480, at the training batch B = 8 and at B = 32, in one process:
    python tools_dev/conv_grouped_train_time.py [out.json] [commit]

Per site: device us of the native forward (fpc_conv2d_grouped, no epilogue), data gradient (fpc_conv2d_grouped_dgrad) and weight
gradient (fpc_conv2d_grouped_wgrad) — every kernel of the call counted, k_pack_grouped and k_wgrad_grouped_reduce included, as the
training step pays them — beside torch's route on the same channel-last tensors in the same run: conv2d(groups=32) and
aten.convolution_backward asked for the input gradient alone and for the weight gradient alone.  Beside them the model's floors
(DESIGN.md 4.2a''): HBM (the operands read once, the result written once, at 5.3 TB/s) and f32 (the multiply-adds at the vector
rate, 78.6 T FMA/s), and the weight gradient's slice count, partial bytes and operand bytes.

Device time per call from torch.profiler's kernel records; the mean of 10 calls after 3 warm-up calls.
Writes profiles/conv_grouped_train_time.json."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.profiler import ProfilerActivity, profile

import fastposecnn_amd.lib  # noqa: F401
from fastposecnn_amd import _native as nat

dev = torch.device("cuda:0")
L = nat.lib()
GROUPS = 32
HBM_TBPS = 5.3
FMA_TPS = 78.6      # 157.3 TFLOP/s of v_fma_f32
# torch's name for the card can be generic ("AMD Radeon Graphics"): the architecture says which chip it is
DEVICE_NAME = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))

# (site, Hi, Wi, C, Cg, stride) of one 640 x 480 frame
SHAPES = [("layer1.conv2", 120, 160, 128, 4, 1), ("layer2.0.conv2", 120, 160, 256, 8, 2), ("layer2.conv2", 60, 80, 256, 8, 1),
          ("layer3.0.conv2", 60, 80, 512, 16, 2), ("layer3.conv2", 30, 40, 512, 16, 1), ("layer4.0.conv2", 30, 40, 1024, 32, 2),
          ("layer4.conv2", 15, 20, 1024, 32, 1)]


def kernel_us(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    tot = 0.0
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            tot += ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
    return tot / reps


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "conv_grouped_train_time.json")
    commit = sys.argv[2] if len(sys.argv) > 2 else None
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for B in (8, 32):
        for site, Hi, Wi, C, Cg, stride in SHAPES:
            Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
            x = torch.randn((B, Hi, Wi, C), device=dev, generator=g)
            w = torch.randn((C, Cg, 3, 3), device=dev, generator=g) / (9 * Cg) ** 0.5
            dy = torch.randn((B, Ho, Wo, C), device=dev, generator=g)
            y = torch.empty((B, Ho, Wo, C), device=dev)
            dx = torch.empty((B, Hi, Wi, C), device=dev)
            dw = torch.empty((C, Cg, 3, 3), device=dev)
            sb_, sh_, sw_, sc_ = x.stride()
            xb, yb, wb = 4.0 * B * Hi * Wi * C, 4.0 * B * Ho * Wo * C, 4.0 * C * Cg * 9
            fma = float(B) * Ho * Wo * C * Cg * 9      # the same count for the forward and both gradients
            wsf = torch.empty(L.fpc_conv2d_grouped_workspace_bytes(C, GROUPS), dtype=torch.uint8, device=dev)
            wsd = torch.empty(L.fpc_conv2d_grouped_dgrad_workspace_bytes(C, GROUPS), dtype=torch.uint8, device=dev)
            nws = L.fpc_conv2d_grouped_wgrad_workspace_bytes(B, Ho, Wo, C, GROUPS)
            wsw = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)
            tiles = B * ((Ho + 7) // 8) * ((Wo + (15 if stride == 1 else 7)) // (16 if stride == 1 else 8))
            nslice = min(nws // (C * Cg * 36), tiles)
            s = nat.stream()

            def fwd():
                nat.check(L.fpc_conv2d_grouped(x.data_ptr(), sb_, sh_, sw_, sc_, w.data_ptr(), None, None, y.data_ptr(), B, Hi, Wi, C,
                                               GROUPS, stride, 0, 0, wsf.data_ptr(), wsf.numel(), s), "fpc_conv2d_grouped")

            def dgrad():
                nat.check(L.fpc_conv2d_grouped_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, Hi, Wi, C, GROUPS, stride,
                                                     wsd.data_ptr(), wsd.numel(), s), "fpc_conv2d_grouped_dgrad")

            def wgrad():
                nat.check(L.fpc_conv2d_grouped_wgrad(x.data_ptr(), sb_, sh_, sw_, dy.data_ptr(), dw.data_ptr(), B, Hi, Wi, C, GROUPS,
                                                     stride, wsw.data_ptr(), wsw.numel(), s), "fpc_conv2d_grouped_wgrad")

            xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)      # channel-last NCHW views
            conv_bwd = torch.ops.aten.convolution_backward

            def t_bwd(mask):
                return lambda: conv_bwd(dyt, xt, w, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], GROUPS, mask)

            with torch.no_grad():
                row = {"site": site, "B": B, "Hi": Hi, "Wi": Wi, "C": C, "Cg": Cg, "stride": stride, "gfma": round(fma / 1e9, 3),
                       "f32_floor_us": round(fma / (FMA_TPS * 1e6), 2),
                       "fwd": {"native_us": round(kernel_us(fwd), 2), "torch_us": round(kernel_us(
                           lambda: torch.nn.functional.conv2d(xt, w, None, stride, 1, 1, GROUPS)), 2),
                           "hbm_floor_us": round((xb + yb + wb) / (HBM_TBPS * 1e6), 2)},
                       "dgrad": {"native_us": round(kernel_us(dgrad), 2), "torch_us": round(kernel_us(t_bwd([True, False, False])), 2),
                                 "hbm_floor_us": round((xb + yb + wb) / (HBM_TBPS * 1e6), 2)},
                       "wgrad": {"native_us": round(kernel_us(wgrad), 2), "torch_us": round(kernel_us(t_bwd([False, True, False])), 2),
                                 "hbm_floor_us": round((xb + yb) / (HBM_TBPS * 1e6), 2), "slices": int(nslice), "tiles": int(tiles),
                                 "partial_mbytes": round((nslice * wb if nslice > 1 else 0.0) / 1e6, 3),
                                 "operand_mbytes": round((xb + yb) / 1e6, 2)}}
            for op in ("fwd", "dgrad", "wgrad"):
                row[op]["native_wins"] = row[op]["native_us"] < row[op]["torch_us"]
            rows.append(row)
            print(f"B={B:2d} {site:16s} C={C:5d} Cg={Cg:3d} s{stride} f32 floor {row['f32_floor_us']:7.1f} | " + " | ".join(
                f"{op} native {row[op]['native_us']:8.1f} torch {row[op]['torch_us']:8.1f} hbm {row[op]['hbm_floor_us']:6.1f}"
                for op in ("fwd", "dgrad", "wgrad")) + f" | slices {nslice}", flush=True)
            del x, w, dy, y, dx, dw, wsf, wsd, wsw
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"device": DEVICE_NAME, "commit": commit,
                   "what": "device us per call, mean of 10 after 3 warm-up, every kernel of the call counted (weight packing and the "
                           "slice reduce included); hbm floor at 5.3 TB/s, f32 floor at 78.6 T FMA/s", "rows": rows}, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
