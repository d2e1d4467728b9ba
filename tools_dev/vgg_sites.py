"""A VGG plan on the MI355X, measured in one process with no pass / fail gate:
python tools_dev/vgg_sites.py [out.json]

1. The two kernels of csrc/vgg.hip stand-alone at the shapes of a 640 x 480 frame, B = 1 and B = 32: features.0 (k_conv3x3_c3) and the
   five 2x2 max-pools (k_maxpool2x2): device time, the bytes the launch must move (what it reads + what it writes), the achieved
   bytes/s, and beside it a device-to-device copy timed in the same run that moves the same number of bytes (it copies half of them:
   a copy reads and writes).
2. The engine on vgg16_bn at 640 x 480, B = 1 and B = 32 (the headline batch, the largest built here), autotuned at split level 3:
   the device time of every launch of a frame in launch order with the plan code of every convolution site, the encoder's share,
   and the wall time per forward (plain launches and graph replay), beside resnet34's forward from the same run.

Device time per launch from torch.profiler's kernel records, the mean of 10 calls after 3 warm-up calls; wall time from device
events around `reps` forwards after a fifth as many.  Writes profiles/vgg16_bn_sites.json and a text table beside it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.profiler import ProfilerActivity, profile

import fastposecnn_amd.lib as lib
from fastposecnn_amd import _native as nat
from fastposecnn_amd import config
from fastposecnn_amd.engine import NetEngine

dev = torch.device("cuda:0")
L = nat.lib()
LINES = []
H, W = 480, 640


def emit(*parts):
    """print, and keep the line for the text table written beside the JSON"""
    line = " ".join(str(p) for p in parts)
    LINES.append(line)
    print(line, flush=True)


def kernel_events(fn, reps=10):
    """[(kernel name, mean device us)] of the launches of one call of fn, in launch order."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    evs = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    evs.sort(key=lambda ev: ev.time_range.start)
    per = len(evs) // reps
    us = lambda ev: ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
    if per * reps != len(evs):      # (not the same launches every call: the sum alone)
        return [("all", sum(us(ev) for ev in evs) / reps)]
    return [(evs[i].name, sum(us(evs[i + r * per]) for r in range(reps)) / reps) for i in range(per)]


def short(name):
    return name.split("(")[0].replace("void fpc::", "").replace("fpc::", "")[:48]


def copy_us(nbytes):
    half = int(nbytes // 8) * 4                      # a copy of half the bytes reads and writes the launch's byte count
    a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
    return sum(t for _, t in kernel_events(lambda: b.copy_(a)))


def kernel_rows(B):
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    p = lambda t: t.data_ptr()
    s = nat.stream()
    x4 = torch.rand((B, H, W, 4), device=dev, generator=g)
    w = torch.randn((64, 3, 3, 3), device=dev, generator=g) * (2.0 / 27) ** 0.5
    sc, sh = torch.rand(64, device=dev, generator=g) + 0.5, torch.randn(64, device=dev, generator=g) * 0.1
    o = torch.empty((B, H, W, 64), device=dev)
    jobs = [("features.0 conv3x3_c3", H, W, 4, 64, lambda: nat.check(L.fpc_conv3x3_c3(p(x4), p(w), p(sc), p(sh), p(o), B, H, W, 64, 1, s), "conv3x3_c3"),
             4.0 * B * H * W * (4 + 64))]
    keep = [x4, o]
    for i, c in enumerate((64, 128, 256, 512, 512)):
        h, ww = H >> i, W >> i
        xi = o if i == 0 else torch.rand((B, h, ww, c), device=dev, generator=g)
        yo = torch.empty((B, h // 2, ww // 2, c), device=dev)
        keep += [xi, yo]
        jobs.append((f"pool{i + 1} maxpool2x2", h, ww, c, c,
                     (lambda xi=xi, yo=yo, h=h, ww=ww, c=c: nat.check(L.fpc_maxpool2x2_fwd(p(xi), p(yo), B, h, ww, c, s), "maxpool2x2")),
                     4.0 * B * h * ww * c * 1.25))
    for name, h, ww, cin, cout, call, nbytes in jobs:
        us = sum(t for _, t in kernel_events(call))
        cu = copy_us(nbytes)
        rows.append({"launch": name, "B": B, "h": h, "w": ww, "Cin": cin, "Cout": cout, "mbytes": round(nbytes / 1e6, 3), "us": round(us, 2),
                     "gbps": round(nbytes / us * 1e-3, 1), "copy_us": round(cu, 2), "copy_gbps": round(nbytes / cu * 1e-3, 1)})
        emit(f"B={B:2d} {name:24s} {h:3d}x{ww:3d} {cin:3d}->{cout:3d} {rows[-1]['mbytes']:9.2f} MB {us:9.1f} us {rows[-1]['gbps']:8.1f} GB/s"
             f"   copy {cu:9.1f} us {rows[-1]['copy_gbps']:8.1f} GB/s")
    del keep, jobs
    torch.cuda.empty_cache()
    return rows


def engine_rows(B, reps):
    out = {}
    x = torch.rand((B, 3, H, W), device=dev)
    for enc in ("vgg16_bn", "resnet34"):
        hp = config.INFERENCE()
        hp.RUNTIME_TIMING = False
        hp.ENCODER = enc
        hp.PERFORM_AGGREGATION = False
        torch.manual_seed(0)
        m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).eval().to(dev)
        row = {}
        eng = NetEngine(m, B, H, W, dev, autotune=True, graph=False, split_precision=3)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for graph in (False, True):           # the same tuned plan, plain launches and then graph replay
                if graph:
                    nat.check(L.fpc_net_set_graph(eng._h, 1), "fpc_net_set_graph")
                for _ in range(max(2, reps // 5)):
                    eng.forward(x, want_logits=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                for _ in range(reps):
                    eng.forward(x, want_logits=False)
                e1.record(side)
                e1.synchronize()
                row["graph_ms" if graph else "plain_ms"] = round(e0.elapsed_time(e1) / reps, 4)
                if not graph:
                    evs = kernel_events(lambda: eng.forward(x, want_logits=False))
                    row["kernels"] = len(evs)
                    row["kernel_ms"] = round(sum(t for _, t in evs) / 1e3, 4)
                    row["gflop"] = round(eng.flops()[0] / 1e9, 2)
                    row["workspace_mb"] = round(L.fpc_net_workspace_bytes(eng._h) / 1e6, 1)
                    row["plans"] = [list(q) for q in eng.conv_plans()]
                    if enc == "vgg16_bn":
                        row["launches_us"] = [[short(n), round(t, 1)] for n, t in evs]
                        # the encoder: everything up to and including the fifth max-pool
                        last = max(i for i, (n, _) in enumerate(evs) if "k_maxpool2x2" in n)
                        row["encoder_kernel_ms"] = round(sum(t for _, t in evs[:last + 1]) / 1e3, 4)
                        row["vgg_kernels_ms"] = round(sum(t for n, t in evs if "k_maxpool2x2" in n or "k_conv3x3_c3" in n) / 1e3, 4)
                    by_name = {}
                    for n, t in evs:
                        by_name[short(n)] = by_name.get(short(n), 0.0) + t
                    row["top_kernels_us"] = {k: round(v, 1) for k, v in sorted(by_name.items(), key=lambda kv: -kv[1])[:8]}
        side.synchronize()
        del eng
        out[enc] = row
        emit(f"B={B:2d} {enc:9s} " + str({k: v for k, v in row.items() if k not in ("launches_us", "plans")}))
        if "launches_us" in row:
            emit(f"B={B:2d} {enc} encoder site plan codes:", [q[2] for q in row["plans"][:12]])
            for i, (n, t) in enumerate(row["launches_us"]):
                emit(f"B={B:2d} {enc} launch {i:3d} {n:48s} {t:9.1f} us")
        del m
        torch.cuda.empty_cache()
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "vgg16_bn_sites.json")
    res = {"device": torch.cuda.get_device_name(0),
           "what": "device us per launch (torch.profiler kernel records, mean of 10 after 3 warm-up); bytes = what the launch reads + what it "
                   "writes; the copy moves the same bytes (copies half); wall ms per forward from device events, without the logits; "
                   "640 x 480",
           "kernels": {}, "forward": {}}
    for B in (1, 32):
        res["kernels"][f"B{B}"] = kernel_rows(B)
    for B, reps in ((1, 50), (32, 10)):
        res["forward"][f"B{B}"] = engine_rows(B, reps)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
