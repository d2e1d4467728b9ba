"""The merge + head passes and the x4 upsample + class compression at 22 classes (k_head_part_wide, k_up4_compress_wide and, with
FPC_UP4_WIDE=0, k_up4_compress<32>) beside the 7-class kernels, at 640 x 480, B = 1 and B = 32, resnet18 with random weights, static
plans, in one process: python tools_dev/wide_classes_time.py [out.json]

Device time per kernel from torch.profiler's kernel records, the mean over `reps` forwards after 3 warm-up forwards.  Rates are on
algorithmic bytes: every map read once, every output written once (the low-resolution taps of the x4 pass count once).  Writes
profiles/wide_classes_time.json."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.profiler import ProfilerActivity, profile

import fastposecnn_amd.lib as L
from fastposecnn_amd import config

dev = torch.device("cuda:0")
H, W = 480, 640


def model(classes):
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet18"
    hp.PERFORM_AGGREGATION = False
    hp.ENGINE_AUTOTUNE = False
    hp.ENGINE_GRAPH = False
    hp.SELECTED_CLASSES = ["bg"] + ["obj%d" % i for i in range(1, classes)]
    torch.manual_seed(0)
    return L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).to(dev).eval()


def kernel_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    tot = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            t = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
            tot[ev.name] = tot.get(ev.name, 0.0) + t
    return {k: v / reps for k, v in tot.items()}


def head_bytes(classes, B):
    G = classes - 1
    chp = sum((c + 3) // 4 * 4 for c in (classes, 4 * G, 3 * G, 3 * G))
    lo_px, hi_px = (H // 8) * (W // 8), (H // 4) * (W // 4)
    low = B * lo_px * (4 * 3 * 128 + chp) * 4
    hi = B * (hi_px * (4 * 128 + chp) + lo_px * chp) * 4
    return low, hi


def up4_bytes(classes, B, logits):
    G = classes - 1
    chp = sum((c + 3) // 4 * 4 for c in (classes, 4 * G, 3 * G, 3 * G))
    n = B * (H // 4) * (W // 4) * chp * 4 + B * H * W * (8 + 10 * 4)      # taps once; i64 labels + 10 categorical planes
    if logits:
        n += B * H * W * (classes + 10 * G) * 4
    return n


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                  "profiles", "wide_classes_time.json")
    rows = []
    for B in (1, 32):
        x = torch.rand((B, 3, H, W), device=dev)
        for classes, generic in ((7, False), (22, False), (22, True)):
            if generic:
                os.environ["FPC_UP4_WIDE"] = "0"
            m = model(classes)
            with torch.no_grad():
                m.pure_model_forward(x)
            os.environ.pop("FPC_UP4_WIDE", None)
            eng = next(iter(m._engines.values()))
            for logits in (True, False):
                ks = kernel_us(lambda: eng.forward(x, want_logits=logits), 20 if B == 1 else 5)
                row = {"B": B, "classes": classes, "logits": logits, "up4_route": "k_up4_compress<32>" if generic else "default",
                       "kernels_us": {}}
                lo_b, hi_b = head_bytes(classes, B)
                for name, us in sorted(ks.items()):
                    short = None
                    if "k_head_part" in name or "k_merge_head" in name:
                        hi = "<true" in name or "ILb1" in name
                        short, nbytes = name, (hi_b if hi else lo_b)
                    elif "k_up4" in name:
                        short, nbytes = name, up4_bytes(classes, B, logits)
                    if short:
                        row["kernels_us"][short] = {"us": round(us, 2), "algorithmic_MB": round(nbytes / 1e6, 2),
                                                    "TB_per_s": round(nbytes / us / 1e6, 3)}
                row["forward_kernels_us_total"] = round(sum(ks.values()), 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del m, eng
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "device us per kernel and forward, mean over 20 (B = 1) / 5 "
                   "(B = 32) forwards after 3 warm-up; resnet18, 640 x 480, static plans; bytes: maps read once, outputs written once",
                   "rows": rows}, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
