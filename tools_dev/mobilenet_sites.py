"""The MobileNetV2 encoder's kernels (csrc/mobilenet.hip, csrc/depthwise.hip) on every encoder site of a 640 x 480 frame, B = 1 and B = 32, and the
whole forward beside resnet18's, in one process: python tools_dev/mobilenet_sites.py [out.json]

Per site (the stem, 17 depthwise, 16 expand, 17 project, the last 1x1 = 52 launches): device time per launch, the bytes the launch
must move (input + output + weights + the residual where there is one), the achieved bytes/s, and beside it a device-to-device copy
timed in the same run that moves the same number of bytes (it copies half of them: a copy reads and writes).  The four widest 1x1
sites also as FLOP/s against the f32 matrix peak (157.3 TFLOP/s).  Then the engine: device time of the encoder's kernels and of the
whole forward from the profiler's kernel records (with the eight kernels that take most of it), and the wall time per forward (plain launches and graph replay) for mobilenet_v2
and resnet18 from the same run.

Device time per call from torch.profiler's kernel records, the mean of 10 calls after 3 warm-up calls; wall time from device events
around 50 forwards after 10.  Writes profiles/mobilenet_v2_sites.json and a text table beside it."""
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
F32_PEAK_TFLOPS = 157.3
SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
ENCODER_KERNELS = ("k_stem3x3s2", "k_dw_fwd", "k_conv1x1_f32")
LINES = []


def emit(*parts):
    """print, and keep the line for the text table written beside the JSON"""
    line = " ".join(str(p) for p in parts)
    LINES.append(line)
    print(line, flush=True)


def sites(H=480, W=640):
    """(name, kind, Hi, Wi, Cin, Cout, stride, act, residual) of every encoder launch, in launch order."""
    out = [("features.0", "stem", H, W, 3, 32, 2, 1, False)]
    h, w, inp, idx = H // 2, W // 2, 32, 1
    for t, c, n, s in SETTING:
        for i in range(n):
            st, hid = (s if i == 0 else 1), inp * t
            if t != 1:
                out.append((f"features.{idx}.expand", "pw", h, w, inp, hid, 1, 1, False))
            out.append((f"features.{idx}.dw", "dw", h, w, hid, hid, st, 1, False))
            h, w = h // st, w // st
            out.append((f"features.{idx}.project", "pw", h, w, hid, c, 1, 0, st == 1 and inp == c))
            inp, idx = c, idx + 1
    out.append(("features.18", "pw", h, w, inp, 1280, 1, 1, False))
    return out


def kernel_events(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    evs = []
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            evs.append((ev.name, (ev.device_time if hasattr(ev, "device_time") else ev.cuda_time) / reps))
    return evs


def kernel_us(fn, reps=10):
    return sum(t for _, t in kernel_events(fn, reps))


def site_rows(B):
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for name, kind, Hi, Wi, Cin, Cout, stride, act, has_res in sites():
        Ho, Wo = Hi // stride, Wi // stride
        cin_layout = 4 if kind == "stem" else Cin
        x = torch.randn((B, Hi, Wi, cin_layout), device=dev, generator=g)
        wn = {"stem": 32 * 27, "dw": Cin * 9, "pw": Cin * Cout}[kind]
        w = torch.randn(wn, device=dev, generator=g) / {"stem": 27, "dw": 9, "pw": Cin}[kind] ** 0.5
        sc = torch.rand(Cout, device=dev, generator=g) + 0.5
        sh = torch.randn(Cout, device=dev, generator=g)
        o = torch.empty((B, Ho, Wo, Cout), device=dev)
        res = torch.randn((B, Ho, Wo, Cout), device=dev, generator=g) if has_res else None
        s = nat.stream()
        if kind == "stem":
            call = lambda: nat.check(L.fpc_stem3x3s2(x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), o.data_ptr(), B, Hi, Wi, 32, s), "stem")
            flop = 2.0 * B * Ho * Wo * 32 * 27
        elif kind == "dw":
            call = lambda: nat.check(L.fpc_dwconv3x3(x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), o.data_ptr(), B, Hi, Wi, Cin, stride, act, s), "dw")
            flop = 2.0 * B * Ho * Wo * Cin * 9
        else:
            call = lambda: nat.check(L.fpc_conv1x1_f32(x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), nat.ptr(res), o.data_ptr(), B * Hi * Wi, Cin, Cout, act, s), "pw")
            flop = 2.0 * B * Ho * Wo * Cin * Cout
        nbytes = 4.0 * (x.numel() + o.numel() + wn + (o.numel() if has_res else 0))
        us = kernel_us(call)
        half = int(nbytes // 8) * 4                      # a copy of half the bytes reads and writes the site's byte count
        a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        copy_us = kernel_us(lambda: b.copy_(a))
        rows.append({"site": name, "kind": kind, "B": B, "Hi": Hi, "Wi": Wi, "Cin": Cin, "Cout": Cout, "stride": stride, "res": has_res,
                     "mbytes": round(nbytes / 1e6, 3), "mflop": round(flop / 1e6, 2), "us": round(us, 2),
                     "gbps": round(nbytes / us * 1e-3, 1), "copy_us": round(copy_us, 2), "copy_gbps": round(nbytes / copy_us * 1e-3, 1),
                     "tflops": round(flop / us * 1e-6, 2)})
        emit(f"B={B:2d} {name:22s} {kind:4s} {Hi:3d}x{Wi:3d} {Cin:4d}->{Cout:4d} s{stride} {rows[-1]['mbytes']:9.2f} MB {us:9.1f} us "
              f"{rows[-1]['gbps']:8.1f} GB/s   copy {copy_us:9.1f} us {rows[-1]['copy_gbps']:8.1f} GB/s   {rows[-1]['tflops']:6.2f} TFLOP/s")
        del x, w, o, res, a, b
    torch.cuda.empty_cache()
    return rows


def engine_rows(B):
    out = {}
    x = torch.rand((B, 3, 480, 640), device=dev)
    for enc in ("mobilenet_v2", "resnet18"):
        hp = config.INFERENCE()
        hp.RUNTIME_TIMING = False
        hp.ENCODER = enc
        hp.PERFORM_AGGREGATION = False
        torch.manual_seed(0)
        m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).eval().to(dev)
        row = {}
        for graph in (False, True):
            eng = NetEngine(m, B, 480, 640, dev, autotune=True, graph=graph, split_precision=3)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(10):
                    eng.forward(x, want_logits=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                for _ in range(50):
                    eng.forward(x, want_logits=False)
                e1.record(side)
                e1.synchronize()
                row["graph_ms" if graph else "plain_ms"] = round(e0.elapsed_time(e1) / 50, 4)
                if not graph:
                    evs = kernel_events(lambda: eng.forward(x, want_logits=False))
                    row["kernels"] = len(evs) // 10
                    row["kernel_ms"] = round(sum(t for _, t in evs) / 1e3, 4)
                    row["encoder_kernel_ms"] = round(sum(t for n, t in evs if any(k in n for k in ENCODER_KERNELS)) / 1e3, 4)
                    row["gflop"] = round(eng.flops()[0] / 1e9, 2)
                    by_name = {}
                    for n, t in evs:
                        key = n.split("(")[0].replace("void fpc::", "")[:60]
                        by_name[key] = by_name.get(key, 0.0) + t
                    row["top_kernels_us"] = {k: round(v, 1) for k, v in sorted(by_name.items(), key=lambda kv: -kv[1])[:8]}
            side.synchronize()
            del eng
        out[enc] = row
        emit(f"B={B:2d} {enc:13s} {row}")
        del m
        torch.cuda.empty_cache()
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "mobilenet_v2_sites.json")
    res = {"device": torch.cuda.get_device_name(0),
           "what": "device us per launch (torch.profiler kernel records, mean of 10 after 3 warm-up); bytes = input + output + weights "
                   "(+ residual); the copy moves the same bytes (copies half); wall ms per forward from device events around 50 "
                   "forwards after 10, without the logits",
           "sites": {}, "forward": {}}
    for B in (1, 32):
        rows = site_rows(B)
        res["sites"][f"B{B}"] = rows
        res["sites"][f"B{B}_total"] = {"us": round(sum(r["us"] for r in rows), 1), "copy_us": round(sum(r["copy_us"] for r in rows), 1),
                                       "mbytes": round(sum(r["mbytes"] for r in rows), 1), "gflop": round(sum(r["mflop"] for r in rows) / 1e3, 3)}
        emit(f"B={B}: total", res["sites"][f"B{B}_total"])
        wide = sorted((r for r in rows if r["kind"] == "pw"), key=lambda r: -r["mflop"])[:4]
        res["sites"][f"B{B}_widest"] = [{"site": r["site"], "tflops": r["tflops"], "share_of_f32_peak": round(r["tflops"] / F32_PEAK_TFLOPS, 3)} for r in wide]
        emit(f"B={B}: widest 1x1 sites", res["sites"][f"B{B}_widest"])
    for B in (1, 32):
        res["forward"][f"B{B}"] = engine_rows(B)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
