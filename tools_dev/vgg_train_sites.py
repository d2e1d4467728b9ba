"""The VGG encoders' training-side kernels (csrc/vgg_train.hip and the forwards they go with) against torch's own:
python tools_dev/vgg_train_sites.py [out.json]

1. Sites.  features.0 (3 -> 64 channels) and the five 2x2 max-pools of vgg16_bn on a 640 x 480 frame at the training batch, 8, forward
   and backward, each through its C entry, beside torch's kernel(s) for the same call in the same process — what the training step
   runs with FPC_TRAIN_NATIVE_VGG unset:
     features.0 forward   fpc_image_nhwc4 + fpc_conv3x3_c3 (shift = bias)      | the channel-last copy of the image + F.conv2d with bias
     features.0 backward  fpc_conv3x3_c3_wgrad (dw and db)                     | aten.convolution_backward, weight and bias asked for
     pool forward         fpc_maxpool2x2_fwd                                   | aten.max_pool2d_with_indices (values + int64 indices)
     pool backward        fpc_maxpool2x2_bwd (arg-max recomputed from x)       | aten.max_pool2d_with_indices_backward
   The two sides ALTERNATE: one sample is `INNER` calls between two device events, a native sample, then a torch sample, ROUNDS
   times after warm-up; the median, minimum and maximum per call are kept.  Bytes = what each side must move (native: operands and
   results; torch: the same plus the index plane written / read and dx's zero fill where aten makes one), computed from the shapes.
2. The step.  One forward + backward of the HEAD_TRAINING model on vgg16_bn at batch 8, 640 x 480 (the loss of the tests: the mean
   square of every output), train_conv.NATIVE_VGG on and off alternating in the same process after both have tuned their plans; median
   of the host clock around a synchronised step, and the counters each setting moved.
Writes profiles/vgg_train_sites.json / .txt."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, H, W = 8, 480, 640
POOL_CHANNELS = (64, 128, 256, 512, 512)      # the pools' inputs: H / 2^i x W / 2^i
ROUNDS, INNER = 9, 4
LINES = []


def emit(*parts):
    line = " ".join(str(p) for p in parts)
    LINES.append(line)
    print(line, flush=True)


def alternate(torch_mod, native, other):
    """(native, torch) lists of us per call: ROUNDS alternating samples of INNER calls each, after two warm-up samples of both"""
    ev = [torch_mod.cuda.Event(enable_timing=True) for _ in range(2)]
    out = ([], [])
    for r in range(ROUNDS + 2):
        for k, fn in enumerate((native, other)):
            ev[0].record()
            for _ in range(INNER):
                fn()
            ev[1].record()
            ev[1].synchronize()
            if r >= 2:
                out[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / INNER)
    return out


def sites():
    import torch
    import torch.nn.functional as F

    from fastposecnn_amd import _native as nat
    dev = torch.device("cuda:0")
    L = nat.lib()
    st = nat.stream()
    p = lambda t: t.data_ptr()
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []

    def row(site, op, native, other, native_bytes, torch_bytes):
        n_us, t_us = alternate(torch, native, other)
        nm, tm = statistics.median(n_us), statistics.median(t_us)
        spread = max(max(n_us) - min(n_us), max(t_us) - min(t_us))
        verdict = "native faster" if nm < tm - spread else ("torch faster" if nm > tm + spread else "tie")
        rows.append({"site": site, "op": op, "native_mbytes": round(native_bytes / 1e6, 2), "torch_mbytes": round(torch_bytes / 1e6, 2),
                     "native_us": [round(nm, 1), round(min(n_us), 1), round(max(n_us), 1)],
                     "torch_us": [round(tm, 1), round(min(t_us), 1), round(max(t_us), 1)],
                     "native_gbps": round(native_bytes / nm * 1e-3, 1), "torch_gbps": round(torch_bytes / tm * 1e-3, 1), "verdict": verdict})
        emit(f"{site:22s} {op:3s}  native {nm:8.1f} us ({min(n_us):8.1f} - {max(n_us):8.1f}) {native_bytes / 1e6:8.1f} MB {rows[-1]['native_gbps']:7.1f} GB/s"
             f"   torch {tm:8.1f} us ({min(t_us):8.1f} - {max(t_us):8.1f}) {torch_bytes / 1e6:8.1f} MB {rows[-1]['torch_gbps']:7.1f} GB/s   {verdict}")

    # features.0
    x = torch.randn((B, 3, H, W), device=dev, generator=g)
    w = torch.randn((64, 3, 3, 3), device=dev, generator=g) * (2.0 / 27) ** 0.5
    bias = torch.randn(64, device=dev, generator=g) * 0.1
    img4 = torch.empty((B, H, W, 4), device=dev)
    y = torch.empty((B, 64, H, W), device=dev).contiguous(memory_format=torch.channels_last)
    gy = torch.randn((B, 64, H, W), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    dw, db = torch.empty_like(w), torch.empty_like(bias)
    ws = nat.workspace("bench_c3_wgrad", dev, L.fpc_conv3x3_c3_wgrad_workspace_bytes(B, H, W))
    px = B * H * W

    def c3_fwd():
        nat.check(L.fpc_image_nhwc4(p(x), p(img4), B, H, W, st), "image")
        nat.check(L.fpc_conv3x3_c3(p(img4), p(w), None, p(bias), p(y), B, H, W, 64, 0, st), "c3")
    xcl = x.contiguous(memory_format=torch.channels_last)
    row("features.0 3->64", "fwd", c3_fwd, lambda: F.conv2d(x.contiguous(memory_format=torch.channels_last), w, bias, 1, 1),
        4.0 * px * (3 + 4 + 4 + 64), 4.0 * px * (3 + 3 + 3 + 64))
    row("features.0 3->64", "bwd",
        lambda: nat.check(L.fpc_conv3x3_c3_wgrad(p(img4), p(gy), p(dw), p(db), B, H, W, p(ws), ws.numel(), st), "c3 wgrad"),
        lambda: torch.ops.aten.convolution_backward(gy, xcl, w, [64], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, True]),
        4.0 * px * (4 + 64), 4.0 * px * (3 + 64 + 64))      # (aten reads dy twice: the weight gradient and the bias reduction)
    got = torch.ops.aten.convolution_backward(gy, xcl, w, [64], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, True])
    emit("features.0 bwd, native against torch's own result: |dw - dw_torch|max %.3e (|dw|max %.3e), |db - db_torch|max %.3e (|db|max %.3e)"
         % ((dw - got[1]).abs().max().item(), got[1].abs().max().item(), (db - got[2]).abs().max().item(), got[2].abs().max().item()))
    del x, xcl, img4, y, gy, got
    torch.cuda.empty_cache()

    # the five pools
    for i, C in enumerate(POOL_CHANNELS):
        h, ww = H >> i, W >> i
        xi = torch.relu(torch.randn((B, C, h, ww), device=dev, generator=g)).contiguous(memory_format=torch.channels_last)
        yo = torch.empty((B, C, h // 2, ww // 2), device=dev).contiguous(memory_format=torch.channels_last)
        gyo = torch.randn((B, C, h // 2, ww // 2), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(xi)
        n_in, n_out = float(xi.numel()), float(yo.numel())
        site = f"pool{i + 1} {h}x{ww} C{C}"
        row(site, "fwd", lambda: nat.check(L.fpc_maxpool2x2_fwd(p(xi), p(yo), B, h, ww, C, st), "pool fwd"),
            lambda: torch.ops.aten.max_pool2d_with_indices(xi, [2, 2], [2, 2]), 4 * (n_in + n_out), 4 * n_in + 12 * n_out)
        yt, idx = torch.ops.aten.max_pool2d_with_indices(xi, [2, 2], [2, 2])
        row(site, "bwd", lambda: nat.check(L.fpc_maxpool2x2_bwd(p(xi), p(gyo), p(dx), B, h, ww, C, st), "pool bwd"),
            lambda: torch.ops.aten.max_pool2d_with_indices_backward(gyo, xi, [2, 2], [2, 2], [0, 0], [1, 1], False, idx),
            4 * (n_in + n_out + n_in), 12 * n_out + 4 * n_in)
        want = torch.ops.aten.max_pool2d_with_indices_backward(gyo, xi, [2, 2], [2, 2], [0, 0], [1, 1], False, idx)
        emit(f"{site}: native forward == aten's: {torch.equal(yo, yt)}, native backward == aten's: {torch.equal(dx, want)}")
        del xi, yo, gyo, dx, yt, idx, want
        torch.cuda.empty_cache()
    for op in ("fwd", "bwd"):
        sel = [r for r in rows if r["op"] == op]
        emit(f"per step, {op}: native {sum(r['native_us'][0] for r in sel):9.1f} us   torch {sum(r['torch_us'][0] for r in sel):9.1f} us   (features.0 + 5 pools, medians)")
    return rows


def step():
    import torch

    import fastposecnn_amd.lib as lib
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    dev = torch.device("cuda:0")
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "vgg16_bn"
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    x = torch.stack([synth.make_image(i, H, W) for i in range(B)]).to(dev)

    def one(native):
        train_conv.NATIVE_VGG = native
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.pure_model_forward(x)
        sum(v.square().mean() for v in out.values()).backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    keep = train_conv.NATIVE_VGG
    try:
        for _ in range(2):      # both settings tune their plans and warm up
            one(True), one(False)
        moved = {}
        for native in (True, False):
            before = dict(train_conv.counters)
            one(native)
            moved["on" if native else "off"] = {k: v - before[k] for k, v in train_conv.counters.items() if v != before[k]}
        ms = ([], [])
        for _ in range(7):
            ms[0].append(one(True))
            ms[1].append(one(False))
    finally:
        train_conv.NATIVE_VGG = keep
    res = {"on_ms": [round(statistics.median(ms[0]), 2), round(min(ms[0]), 2), round(max(ms[0]), 2)],
           "off_ms": [round(statistics.median(ms[1]), 2), round(min(ms[1]), 2), round(max(ms[1]), 2)], "counters": moved}
    emit(f"vgg16_bn forward + backward, batch {B}, {W} x {H}: NATIVE_VGG on {res['on_ms'][0]:.2f} ms ({res['on_ms'][1]:.2f} - {res['on_ms'][2]:.2f})"
         f"   off {res['off_ms'][0]:.2f} ms ({res['off_ms'][1]:.2f} - {res['off_ms'][2]:.2f})   median, min - max of 7 alternating steps")
    emit("counters moved by one step, on:", moved["on"])
    emit("counters moved by one step, off:", moved["off"])
    return res


if __name__ == "__main__":
    import torch
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vgg_train_sites.json")
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    rows = sites()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame": [H, W], "encoder": "vgg16_bn",
           "what": f"sites: us per call between device events, {INNER} calls a sample, native and torch samples alternating, median / min / max "
                   f"of {ROUNDS} samples after 2 warm-up samples; bytes from the shapes; verdict: the medians differ by more than the larger "
                   "min-max spread.  step: host clock around a synchronised forward + backward, the two settings alternating",
           "rows": rows, "step": step()}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)
