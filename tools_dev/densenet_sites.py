"""The DenseNet encoders' kernels (csrc/densenet.hip) on every distinct dense op of a densenet121 frame of 640 x 480, B = 1 and B = 32,
and the whole forward beside resnet34's, mobilenet_v2's and efficientnet-b0's, in one process:
python tools_dev/densenet_sites.py [out.json]

Per distinct site (the place step; per dense layer its pre-activated 1x1, one per K; per block its 3x3, the same launch for every
layer of the block but for c0; per transition norm + pool and the 1x1 on the pooled tensor; norm5): device time, the bytes the launch
must move (the channels it reads + the channels it writes + weights and affines), the achieved bytes/s, beside it a device-to-device
copy timed in the same run that moves the same number of bytes (it copies half of them: a copy reads and writes), and FLOP/s against
the f32 matrix peak (157.3 TFLOP/s).  Then the engine: device time of the dense ops' kernels and of the whole forward from the
profiler's kernel records (with the eight kernels that take most of it), and the wall time per forward (plain launches and graph
replay) for the four encoders from the same run.

Device time per call from torch.profiler's kernel records, the mean of 10 calls after 3 warm-up calls; wall time from device events
around 50 forwards after 10.  Writes profiles/densenet121_sites.json and a text table beside it."""
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
LAYERS = (6, 12, 24, 16)
DENSE_KERNELS = ("k_dense_",)
LINES = []


def emit(*parts):
    """print, and keep the line for the text table written beside the JSON"""
    line = " ".join(str(p) for p in parts)
    LINES.append(line)
    print(line, flush=True)


def sites(H=480, W=640):
    """(name, kind, h, w, K, Cout, ldi, ldo, launches per frame) of every distinct dense op, in launch order."""
    h, w, c = H // 4, W // 4, 64
    out = [("place", "place", h, w, 64, 64, 64, 64 + 32 * LAYERS[0], 1)]
    for b, layers in enumerate(LAYERS, 1):
        cend = c + 32 * layers
        for j in range(layers):
            out.append((f"block{b}.layer{j + 1}.pw", "pw", h, w, c + 32 * j, 128, cend, 128, 1))
        out.append((f"block{b}.conv3x3", "conv3", h, w, 128, 32, 128, cend, layers))
        c = cend
        if b < 4:
            out.append((f"transition{b}.norm_pool", "normpool", h, w, c, c, c, c, 1))
            h, w = h // 2, w // 2
            out.append((f"transition{b}.pw", "tpw", h, w, c, c // 2, c, c // 2 + 32 * LAYERS[b], 1))
            c //= 2
        else:
            out.append(("norm5", "norm", h, w, c, c, c, c, 1))
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
    for name, kind, h, w, K, Cout, ldi, ldo, count in sites():
        M = B * h * w
        s = nat.stream()
        x = torch.randn((M, ldi), device=dev, generator=g)
        s1, t1 = torch.rand(K, device=dev, generator=g) + 0.5, torch.randn(K, device=dev, generator=g)
        form = -1
        if kind == "place":
            o = torch.empty((M, ldo), device=dev)
            call = lambda: nat.check(L.fpc_dense_place(p(x), p(o), M, 64, ldo, s), "place")
            moved, flop = 2.0 * M * 64, 0.0
        elif kind in ("pw", "tpw"):
            o = torch.empty((M, ldo), device=dev)
            wt = torch.randn((Cout, K), device=dev, generator=g) / K ** 0.5
            s2, t2 = torch.rand(Cout, device=dev, generator=g) + 0.5, torch.randn(Cout, device=dev, generator=g)
            pre = kind == "pw"
            call = lambda: nat.check(L.fpc_dense_pw(p(x), p(s1) if pre else None, p(t1) if pre else None, p(wt), p(s2) if pre else None,
                                                    p(t2) if pre else None, p(o), M, K, Cout, ldi, ldo, 1 if pre else 0, -1, s), "pw")
            moved, flop = 1.0 * M * (K + Cout) + Cout * K + 2 * (K + Cout), 2.0 * M * K * Cout
            form = L.fpc_dense_pw_form(M, K, Cout)
        elif kind == "conv3":
            o = torch.empty((M, ldo), device=dev)
            w4 = torch.randn((32, 128, 3, 3), device=dev, generator=g) / 1152 ** 0.5
            wt = torch.empty(9 * 32 * 128, device=dev)
            nat.check(L.fpc_dense_conv3x3_pack(p(w4), p(wt), s), "pack")
            call = lambda: nat.check(L.fpc_dense_conv3x3(p(x), p(wt), p(o), B, h, w, ldo - 32, ldo, -1, s), "conv3")
            moved, flop = 1.0 * M * (128 + 32) + 9 * 32 * 128, 2.0 * M * 1152 * 32
            form = L.fpc_dense_conv3x3_form(B, h, w)
        else:
            o = torch.empty((M, K), device=dev)
            pooled = torch.empty((M // 4, K), device=dev) if kind == "normpool" else None
            call = lambda: nat.check(L.fpc_dense_norm_pool(p(x), p(s1), p(t1), p(o), nat.ptr(pooled), B, h, w, K, 1 if pooled is not None else 0, s),
                                     "norm_pool")
            moved, flop = (2.25 if kind == "normpool" else 2.0) * M * K, 0.0
        nbytes = 4.0 * moved
        us = kernel_us(call)
        half = int(nbytes // 8) * 4                      # a copy of half the bytes reads and writes the site's byte count
        a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        copy_us = kernel_us(lambda: b.copy_(a))
        rows.append({"site": name, "kind": kind, "B": B, "h": h, "w": w, "K": K, "Cout": Cout, "ldi": ldi, "ldo": ldo, "form": form,
                     "per_frame": count, "mbytes": round(nbytes / 1e6, 3), "mflop": round(flop / 1e6, 2), "us": round(us, 2),
                     "gbps": round(nbytes / us * 1e-3, 1), "copy_us": round(copy_us, 2), "copy_gbps": round(nbytes / copy_us * 1e-3, 1),
                     "tflops": round(flop / us * 1e-6, 2), "share_of_f32_peak": round(flop / us * 1e-6 / F32_PEAK_TFLOPS, 4)})
        emit(f"B={B:2d} {name:24s} {kind:8s} {h:3d}x{w:3d} {K:4d}->{Cout:4d} ld {ldi:4d}/{ldo:4d} f{form:2d} x{count:2d} {rows[-1]['mbytes']:9.2f} MB "
             f"{us:9.1f} us {rows[-1]['gbps']:8.1f} GB/s   copy {copy_us:9.1f} us   {rows[-1]['tflops']:6.2f} TFLOP/s "
             f"({100 * rows[-1]['share_of_f32_peak']:.1f}% of the f32 matrix peak)")
        del x, o, a, b
    torch.cuda.empty_cache()
    return rows


def engine_rows(B):
    out = {}
    x = torch.rand((B, 3, 480, 640), device=dev)
    for enc in ("densenet121", "resnet34", "mobilenet_v2", "efficientnet-b0"):
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
                    if enc == "densenet121":
                        row["dense_kernel_ms"] = round(sum(t for n, t in evs if any(k in n for k in DENSE_KERNELS)) / 1e3, 4)
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "densenet121_sites.json")
    res = {"device": torch.cuda.get_device_name(0),
           "what": "device us per entry call (torch.profiler kernel records, mean of 10 after 3 warm-up); bytes = the channels read + the "
                   "channels written + weights and affines; the copy moves the same bytes (copies half); per_frame = launches of this shape "
                   "in a frame; wall ms per forward from device events around 50 forwards after 10, without the logits",
           "sites": {}, "forward": {}}
    for B in (1, 32):
        rows = site_rows(B)
        res["sites"][f"B{B}"] = rows
        tot = lambda sel, key: round(sum(r[key] * r["per_frame"] for r in sel), 1)
        res["sites"][f"B{B}_total"] = {"launches": sum(r["per_frame"] for r in rows), "us": tot(rows, "us"), "copy_us": tot(rows, "copy_us"),
                                       "mbytes": tot(rows, "mbytes"), "gflop": round(tot(rows, "mflop") / 1e3, 3)}
        emit(f"B={B}: total over a frame's launches", res["sites"][f"B{B}_total"])
        for kind in ("place", "pw", "conv3", "normpool", "tpw", "norm"):
            sel = [r for r in rows if r["kind"] == kind]
            res["sites"][f"B{B}_{kind}"] = {"launches": sum(r["per_frame"] for r in sel), "us": tot(sel, "us"), "copy_us": tot(sel, "copy_us")}
            emit(f"B={B}: {kind}", res["sites"][f"B{B}_{kind}"])
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
