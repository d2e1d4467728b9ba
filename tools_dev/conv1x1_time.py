"""k_conv1x1 (pointwise.hip) against the best k_conv_igemm bf16 x 3 tiling on every 1x1 shape of ResNet-50 at 640 x 480, B = 1
and B = 32, in one process, through fpc_conv2d: python tools_dev/conv1x1_time.py [out.json]

Device time per call from torch.profiler's kernel records (the weight packing fpc_conv2d does on every call is left out); the
median of 10 calls after 3 warm-up calls.  Writes profiles/conv1x1_time.json."""
import ctypes
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

# (site, Hi, Wi, Cin, Cout, stride, epilogue) of one 640 x 480 frame
SHAPES = [
    ("layer1.0.conv1", 120, 160, 64, 64, 1, "bn_relu"), ("layer1.conv1", 120, 160, 256, 64, 1, "bn_relu"),
    ("layer1.conv3", 120, 160, 64, 256, 1, "bn_res_relu"), ("layer1.0.downsample", 120, 160, 64, 256, 1, "bn"),
    ("layer2.0.conv1", 120, 160, 256, 128, 1, "bn_relu"), ("layer2.conv1", 60, 80, 512, 128, 1, "bn_relu"),
    ("layer2.conv3", 60, 80, 128, 512, 1, "bn_res_relu"), ("layer2.0.downsample", 120, 160, 256, 512, 2, "bn"),
    ("layer3.0.conv1", 60, 80, 512, 256, 1, "bn_relu"), ("layer3.conv1", 30, 40, 1024, 256, 1, "bn_relu"),
    ("layer3.conv3", 30, 40, 256, 1024, 1, "bn_res_relu"), ("layer3.0.downsample", 60, 80, 512, 1024, 2, "bn"),
    ("layer4.0.conv1", 30, 40, 1024, 512, 1, "bn_relu"), ("layer4.conv1", 15, 20, 2048, 512, 1, "bn_relu"),
    ("layer4.conv3", 15, 20, 512, 2048, 1, "bn_res_relu"), ("layer4.0.downsample", 30, 40, 1024, 2048, 2, "bn"),
    ("p5", 15, 20, 2048, 256, 1, "bias"), ("p4.skip_conv", 30, 40, 1024, 256, 1, "bias_up"),
    ("p3.skip_conv", 60, 80, 512, 256, 1, "bias_up"), ("p2.skip_conv", 120, 160, 256, 256, 1, "bias_up"),
]


def requests(B, Cout):
    out = [("k_conv1x1 v0", 0, 0, 4000), ("k_conv1x1 v1", 0, 0, 4001)]
    for bm in (64, 128):
        for bn in (64, 128):
            if bn == 128 and Cout <= 64:
                continue
            for ns in ((1, 2, 4, 8) if B == 1 else (1, 2)):
                out.append((f"k_conv_igemm bf3 {bm}x{bn} split {ns}", bm, bn, 1000 + ns))
    return out


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
        if ev.device_type == torch.autograd.DeviceType.CUDA and "pack_weight" not in ev.name:
            tot += ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
    return tot / reps


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                  "profiles", "conv1x1_time.json")
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for B in (1, 32):
        for site, Hi, Wi, Cin, Cout, stride, extra in SHAPES:
            Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
            x = torch.randn((B, Hi, Wi, Cin), device=dev, generator=g)
            w = torch.randn((Cout, Cin, 1, 1), device=dev, generator=g) / Cin ** 0.5
            o = torch.empty((B, Ho, Wo, Cout), device=dev)
            sc = torch.rand(Cout, device=dev, generator=g) + 0.5 if "bn" in extra else None
            sh = torch.randn(Cout, device=dev, generator=g)
            res = torch.randn((B, Ho, Wo, Cout), device=dev, generator=g) if "res" in extra else None
            up = torch.randn((B, Ho // 2, Wo // 2, Cout), device=dev, generator=g) if "up" in extra else None
            sb_, sh_, sw_, sc_ = x.stride()
            row = {"site": site, "B": B, "M": B * Ho * Wo, "N": Cout, "K": Cin, "stride": stride, "epilogue": extra,
                   "gflop": 2.0 * B * Ho * Wo * Cout * Cin / 1e9, "candidates": {}}
            plan = (ctypes.c_int * 4)()
            for name, bm, bn, ns in requests(B, Cout):
                if ns < 4000 and (L.fpc_conv2d_plan(B, Ho, Wo, Cin, Cout, 1, 1, bm, bn, ns, plan) != 0 or
                                  (plan[0], plan[1], plan[2]) != (bm, bn, ns - 1000)):
                    continue                         # a tiling the planner cannot make for this shape (e.g. more slices than K-steps)
                nb = L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, Cin, Cout, 1, 1, bm, bn, ns)
                if nb > (24 << 30):
                    continue
                ws = torch.empty(nb, dtype=torch.uint8, device=dev)

                def call():
                    nat.check(L.fpc_conv2d(x.data_ptr(), sb_, sh_, sw_, sc_, w.data_ptr(), nat.ptr(sc), nat.ptr(sh), nat.ptr(res),
                                           nat.ptr(up), o.data_ptr(), None, B, Hi, Wi, Cin, Cout, 1, 1, stride, 0,
                                           int("relu" in extra), bm, bn, ns, ws.data_ptr(), ws.numel(), nat.stream()), name)
                row["candidates"][name] = round(kernel_us(call), 2)
                del ws
            pw = {k: v for k, v in row["candidates"].items() if k.startswith("k_conv1x1")}
            ig = {k: v for k, v in row["candidates"].items() if k.startswith("k_conv_igemm")}
            bp, bi = min(pw, key=pw.get), min(ig, key=ig.get)
            row.update(best_conv1x1=bp, best_conv1x1_us=pw[bp], best_igemm=bi, best_igemm_us=ig[bi],
                       speedup=round(ig[bi] / pw[bp], 3), conv1x1_tflops=round(row["gflop"] / pw[bp] * 1e-3, 1))
            rows.append(row)
            print(f"B={B:2d} {site:22s} M={row['M']:7d} N={Cout:5d} K={Cin:5d} s{stride}  k_conv1x1 {pw[bp]:9.1f} us ({bp[-2:]})"
                  f"  igemm {ig[bi]:9.1f} us ({bi[13:]})  x{row['speedup']:.2f}", flush=True)
            del x, w, o, res, up
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "device us per call, mean of 10 after 3 warm-up; "
                   "weight packing excluded", "rows": rows}, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
