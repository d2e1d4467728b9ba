"""The EfficientNet-B0 encoder's kernels (csrc/efficientnet.hip, csrc/depthwise.hip and the gated / swish instantiations of
csrc/mobilenet.hip) on every encoder launch of a 640 x 480 frame, B = 1 and B = 32, and the whole forward beside resnet18's and
mobilenet_v2's, in one process:
python tools_dev/efficientnet_sites.py [out.json]

Per launch (the stem and, per MBConv block, expand — not block 0 —, depthwise, gate and project: 1 + 15 + 16 + 16 + 16 = 64 entry
calls, 80 kernel launches since a gate is two): device time, the bytes the launch must move (input + output + weights + the
residual or the gate where there is one), the achieved bytes/s, and beside it a device-to-device copy timed in the same run that
moves the same number of bytes (it copies half of them: a copy reads and writes).  The four widest 1x1 sites also as FLOP/s against
the f32 matrix peak (157.3 TFLOP/s).  Then the engine: device time of the encoder's kernels and of the whole forward from the
profiler's kernel records (with the eight kernels that take most of it), and the wall time per forward (plain launches and graph
replay) for efficientnet-b0, mobilenet_v2 and resnet18 from the same run.

Device time per call from torch.profiler's kernel records, the mean of 10 calls after 3 warm-up calls; wall time from device events
around 50 forwards after 10.  Writes profiles/efficientnet_b0_sites.json and a text table beside it."""
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
# (repeat, kernel, stride, expand ratio, input, output)
BLOCKS = [(1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80), (3, 5, 1, 6, 80, 112),
          (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)]
ENCODER_KERNELS = {"efficientnet-b0": ("k_stem3x3s2", "k_dw_fwd", "k_mb_pool", "k_mb_excite", "k_conv1x1_f32"),
                   "mobilenet_v2": ("k_stem3x3s2", "k_dw_fwd", "k_conv1x1_f32")}
SWISH = 2
LINES = []


def emit(*parts):
    """print, and keep the line for the text table written beside the JSON"""
    line = " ".join(str(p) for p in parts)
    LINES.append(line)
    print(line, flush=True)


def sites(H=480, W=640):
    """(name, kind, Hi, Wi, Cin, Cout, k, stride, act, residual, Cs) of every encoder entry call, in launch order."""
    out = [("_conv_stem", "stem", H, W, 3, 32, 3, 2, SWISH, False, 0)]
    h, w, idx = H // 2, W // 2, 0
    for repeat, k, stride, expand, cin, cout in BLOCKS:
        for i in range(repeat):
            inp, st = (cin if i == 0 else cout), (stride if i == 0 else 1)
            hid, cs = inp * expand, max(1, inp // 4)
            if expand != 1:
                out.append((f"_blocks.{idx}.expand", "pw", h, w, inp, hid, 1, 1, SWISH, False, 0))
            out.append((f"_blocks.{idx}.dw{k}", "dw", h, w, hid, hid, k, st, SWISH, False, 0))
            h, w = h // st, w // st
            out.append((f"_blocks.{idx}.gate", "gate", h, w, hid, hid, 1, 1, 0, False, cs))
            out.append((f"_blocks.{idx}.project", "gpw", h, w, hid, cout, 1, 1, 0, st == 1 and inp == cout, 0))
            idx += 1
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
    p = lambda t: t.data_ptr()
    for name, kind, Hi, Wi, Cin, Cout, k, stride, act, has_res, Cs in sites():
        Ho, Wo = Hi // stride, Wi // stride
        x = torch.randn((B, Hi, Wi, 4 if kind == "stem" else Cin), device=dev, generator=g)
        wn = {"stem": 32 * 27, "dw": Cin * k * k, "pw": Cin * Cout, "gpw": Cin * Cout, "gate": 2 * Cin * Cs + Cin + Cs}[kind]
        w = torch.randn(wn, device=dev, generator=g) / {"stem": 27, "dw": k * k, "pw": Cin, "gpw": Cin, "gate": Cin}[kind] ** 0.5
        sc = torch.rand(Cout, device=dev, generator=g) + 0.5
        sh = torch.randn(Cout, device=dev, generator=g)
        s = nat.stream()
        extra = 0
        if kind == "gate":
            o = torch.empty((B, Cin), device=dev)
            scratch = torch.empty(L.fpc_mbconv_gate_scratch_floats(B, Hi, Wi, Cin), device=dev)
            w1, b1, w2, b2 = w[:Cs * Cin], w[2 * Cs * Cin:2 * Cs * Cin + Cs], w[Cs * Cin:2 * Cs * Cin], w[2 * Cs * Cin + Cs:]
            b1, b2 = b1.clone(), b2.clone()                   # (16-byte alignment of their own)
            call = lambda: nat.check(L.fpc_mbconv_gate(p(x), p(w1), p(b1), p(w2), p(b2), p(o), p(scratch), B, Hi, Wi, Cin, Cs, s), "gate")
            flop = 1.0 * B * Hi * Wi * Cin + 4.0 * B * Cin * Cs
        else:
            o = torch.empty((B, Ho, Wo, Cout), device=dev)
            res = torch.randn((B, Ho, Wo, Cout), device=dev, generator=g) if has_res else None
            gate = torch.rand((B, Cin), device=dev, generator=g) if kind == "gpw" else None
            extra = (o.numel() if has_res else 0) + (gate.numel() if gate is not None else 0)
            if kind == "stem":
                call = lambda: nat.check(L.fpc_mbconv_stem(p(x), p(w), p(sc), p(sh), p(o), B, Hi, Wi, 32, s), "stem")
                flop = 2.0 * B * Ho * Wo * 32 * 27
            elif kind == "dw":
                call = lambda: nat.check(L.fpc_mbconv_dw(p(x), p(w), p(sc), p(sh), p(o), B, Hi, Wi, Cin, k, stride, act, s), "dw")
                flop = 2.0 * B * Ho * Wo * Cin * k * k
            else:
                call = lambda: nat.check(L.fpc_mbconv_pw(p(x), nat.ptr(gate), p(w), p(sc), p(sh), nat.ptr(res), p(o), B, Hi * Wi, Cin, Cout,
                                                         act, s), "pw")
                flop = 2.0 * B * Ho * Wo * Cin * Cout
        nbytes = 4.0 * (x.numel() + o.numel() + wn + extra)
        us = kernel_us(call)
        half = int(nbytes // 8) * 4                      # a copy of half the bytes reads and writes the site's byte count
        a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        copy_us = kernel_us(lambda: b.copy_(a))
        form = L.fpc_mbconv_pw_form(B, Hi * Wi, Cin, Cout) if kind in ("pw", "gpw") else -1
        rows.append({"site": name, "kind": kind, "B": B, "Hi": Hi, "Wi": Wi, "Cin": Cin, "Cout": Cout, "k": k, "stride": stride,
                     "res": has_res, "form": form, "mbytes": round(nbytes / 1e6, 3), "mflop": round(flop / 1e6, 2), "us": round(us, 2),
                     "gbps": round(nbytes / us * 1e-3, 1), "copy_us": round(copy_us, 2), "copy_gbps": round(nbytes / copy_us * 1e-3, 1),
                     "tflops": round(flop / us * 1e-6, 2)})
        emit(f"B={B:2d} {name:20s} {kind:4s} {Hi:3d}x{Wi:3d} {Cin:4d}->{Cout:4d} s{stride} f{form:2d} {rows[-1]['mbytes']:9.2f} MB {us:9.1f} us "
             f"{rows[-1]['gbps']:8.1f} GB/s   copy {copy_us:9.1f} us {rows[-1]['copy_gbps']:8.1f} GB/s   {rows[-1]['tflops']:6.2f} TFLOP/s")
        del x, w, o, a, b
    torch.cuda.empty_cache()
    return rows


def engine_rows(B):
    out = {}
    x = torch.rand((B, 3, 480, 640), device=dev)
    for enc in ("efficientnet-b0", "mobilenet_v2", "resnet18"):
        hp = config.INFERENCE()
        hp.RUNTIME_TIMING = False
        hp.ENCODER = enc
        hp.PERFORM_AGGREGATION = False
        torch.manual_seed(0)
        m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).eval().to(dev)
        row = {}
        eng = NetEngine(m, B, 480, 640, dev, autotune=True, graph=False, split_precision=3)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for graph in (False, True):           # the same tuned plan, plain launches and then graph replay
                if graph:
                    nat.check(L.fpc_net_set_graph(eng._h, 1), "fpc_net_set_graph")
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
                    if enc in ENCODER_KERNELS:
                        row["encoder_kernel_ms"] = round(sum(t for n, t in evs if any(k in n for k in ENCODER_KERNELS[enc])) / 1e3, 4)
                    row["gflop"] = round(eng.flops()[0] / 1e9, 2)
                    by_name = {}
                    for n, t in evs:
                        key = n.split("(")[0].replace("void fpc::", "")[:60]
                        by_name[key] = by_name.get(key, 0.0) + t
                    row["top_kernels_us"] = {k: round(v, 1) for k, v in sorted(by_name.items(), key=lambda kv: -kv[1])[:8]}
        side.synchronize()
        del eng
        out[enc] = row
        emit(f"B={B:2d} {enc:15s} {row}")
        del m
        torch.cuda.empty_cache()
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "efficientnet_b0_sites.json")
    res = {"device": torch.cuda.get_device_name(0),
           "what": "device us per entry call (torch.profiler kernel records, mean of 10 after 3 warm-up; a gate is two kernels); bytes = "
                   "input + output + weights (+ residual, + gate); the copy moves the same bytes (copies half); wall ms per forward "
                   "from device events around 50 forwards after 10, without the logits",
           "sites": {}, "forward": {}}
    for B in (1, 32):
        rows = site_rows(B)
        res["sites"][f"B{B}"] = rows
        res["sites"][f"B{B}_total"] = {"us": round(sum(r["us"] for r in rows), 1), "copy_us": round(sum(r["copy_us"] for r in rows), 1),
                                       "mbytes": round(sum(r["mbytes"] for r in rows), 1), "gflop": round(sum(r["mflop"] for r in rows) / 1e3, 3)}
        emit(f"B={B}: total", res["sites"][f"B{B}_total"])
        for kind in ("stem", "pw", "dw", "gate", "gpw"):
            sel = [r for r in rows if r["kind"] == kind]
            res["sites"][f"B{B}_{kind}"] = {"calls": len(sel), "us": round(sum(r["us"] for r in sel), 1), "copy_us": round(sum(r["copy_us"] for r in sel), 1)}
            emit(f"B={B}: {kind}", res["sites"][f"B{B}_{kind}"])
        wide = sorted((r for r in rows if r["kind"] in ("pw", "gpw")), key=lambda r: -r["mflop"])[:4]
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
