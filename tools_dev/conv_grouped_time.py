"""k_conv3x3_grouped (conv_grouped.hip) on the seven conv2 site shapes of ResNeXt-50-32x4d at 640 x 480, B = 32 and B = 1, in one
process: python tools_dev/conv_grouped_time.py [out.json]

Per site: the new kernel per form (fpc_conv2d_grouped), the site's HBM floor (bytes in + out + weights at 5.3 TB/s), the best of
the dense routes fpc_conv2d has to the same numbers (the block-diagonal dense expansion of the same weights, C -> C, 3x3: Winograd
forms at stride 1, implicit-GEMM tilings on f32 / bf16 x 3 / fp16 x 2 products; fpc_conv2d's kernels are the parent's, untouched),
and, for information, torch's conv2d(groups=32) on channel-last tensors.

Device time per call from torch.profiler's kernel records (weight packing left out); the mean of 10 calls after 3 warm-up calls.
Writes profiles/conv_grouped_time.json."""
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

# (site, Hi, Wi, C, Cg, stride) of one 640 x 480 frame
SHAPES = [("layer1.conv2", 120, 160, 128, 4, 1), ("layer2.0.conv2", 120, 160, 256, 8, 2), ("layer2.conv2", 60, 80, 256, 8, 1),
          ("layer3.0.conv2", 60, 80, 512, 16, 2), ("layer3.conv2", 30, 40, 512, 16, 1), ("layer4.0.conv2", 30, 40, 1024, 32, 2),
          ("layer4.conv2", 15, 20, 1024, 32, 1)]
FORMS = [0]


def kernel_us(fn, reps=10, skip=("pack",)):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    tot = 0.0
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA and not any(s in ev.name for s in skip):
            tot += ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
    return tot / reps


def dense_requests(B, stride):
    out = []
    if stride == 1:
        out += [("winograd -1", 0, 0, -1), ("winograd -5", 0, 0, -5), ("winograd -7", 0, 0, -7), ("winograd -9", 0, 0, -9)]
    for ns in ((1, 2, 4) if B == 1 else (1,)):
        out += [(f"igemm f32 split {ns}", 0, 0, ns), (f"igemm bf16x3 split {ns}", 0, 0, 1000 + ns), (f"igemm fp16x2 split {ns}", 0, 0, 6000 + ns)]
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "conv_grouped_time.json")
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for B in (32, 1):
        for site, Hi, Wi, C, Cg, stride in SHAPES:
            Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
            x = torch.randn((B, Hi, Wi, C), device=dev, generator=g)
            w = torch.randn((C, Cg, 3, 3), device=dev, generator=g) / (9 * Cg) ** 0.5
            o = torch.empty((B, Ho, Wo, C), device=dev)
            sc = torch.rand(C, device=dev, generator=g) + 0.5
            sh = torch.randn(C, device=dev, generator=g)
            sb_, sh_, sw_, sc_ = x.stride()
            nbytes = 4.0 * (B * Hi * Wi * C + B * Ho * Wo * C + C * Cg * 9)
            row = {"site": site, "B": B, "Hi": Hi, "Wi": Wi, "C": C, "Cg": Cg, "stride": stride,
                   "gflop": 2.0 * B * Ho * Wo * C * Cg * 9 / 1e9, "mbytes": round(nbytes / 1e6, 2),
                   "hbm_floor_us": round(nbytes / (HBM_TBPS * 1e6), 2), "grouped": {}, "dense": {}}
            ws = torch.empty(L.fpc_conv2d_grouped_workspace_bytes(C, GROUPS), dtype=torch.uint8, device=dev)
            for form in FORMS:
                def call():
                    nat.check(L.fpc_conv2d_grouped(x.data_ptr(), sb_, sh_, sw_, sc_, w.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                                   o.data_ptr(), B, Hi, Wi, C, GROUPS, stride, 1, form, ws.data_ptr(), ws.numel(),
                                                   nat.stream()), "fpc_conv2d_grouped")
                row["grouped"][f"form {form}"] = round(kernel_us(call), 2)
            # the dense expansion: zeros outside the block diagonal
            wd = torch.zeros((C, C, 3, 3), device=dev)
            for gi in range(GROUPS):
                wd[gi * Cg:(gi + 1) * Cg, gi * Cg:(gi + 1) * Cg] = w[gi * Cg:(gi + 1) * Cg]
            for name, bm, bn, ns in dense_requests(B, stride):
                nb = L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, C, C, 3, 3, bm, bn, ns)
                if nb == 0 or nb > (16 << 30):
                    continue
                wsd = torch.empty(nb, dtype=torch.uint8, device=dev)

                def dcall():
                    return L.fpc_conv2d(x.data_ptr(), sb_, sh_, sw_, sc_, wd.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, None,
                                        o.data_ptr(), None, B, Hi, Wi, C, C, 3, 3, stride, 1, 1, bm, bn, ns, wsd.data_ptr(),
                                        wsd.numel(), nat.stream())
                if dcall() != 0:          # a request the launcher refuses for this shape
                    torch.cuda.synchronize()
                    continue
                row["dense"][name] = round(kernel_us(dcall, skip=("pack", "absmax")), 2)
                del wsd
            xt = x.permute(0, 3, 1, 2)      # channel-last NCHW view
            with torch.no_grad():
                row["torch_grouped_us"] = round(kernel_us(lambda: torch.nn.functional.conv2d(xt, w, None, stride, 1, 1, GROUPS), skip=()), 2)
            bg = min(row["grouped"], key=row["grouped"].get)
            bd = min(row["dense"], key=row["dense"].get)
            row.update(best_grouped=bg, best_grouped_us=row["grouped"][bg], best_dense=bd, best_dense_us=row["dense"][bd],
                       speedup_vs_dense=round(row["dense"][bd] / row["grouped"][bg], 2),
                       grouped_tflops=round(row["gflop"] / row["grouped"][bg] * 1e3, 1),
                       grouped_tbps=round(nbytes / row["grouped"][bg] * 1e-6, 2))
            rows.append(row)
            print(f"B={B:2d} {site:16s} C={C:5d} Cg={Cg:3d} s{stride}  grouped {row['best_grouped_us']:9.1f} us  floor "
                  f"{row['hbm_floor_us']:8.1f} us  dense {row['best_dense_us']:9.1f} us ({bd})  torch {row['torch_grouped_us']:9.1f} us",
                  flush=True)
            del x, w, wd, o, ws
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "device us per call, mean of 10 after 3 warm-up; weight "
                   "packing excluded; hbm floor at 5.3 TB/s", "rows": rows}, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
