"""The EfficientNet-B0 encoder's depthwise gradient kernels (and the forward they go with) against torch's own:
python tools_dev/efficientnet_train_sites.py [out.json]

Every distinct depthwise site of a 640 x 480 frame at the training batch, 8 (csrc/depthwise.hip: k_dw_fwd with the identity
scale / shift forward, its gradient kernels backward, each through its C entry): forward, data gradient and weight gradient each
beside torch's kernel(s) for the same call in the same process — F.conv2d(groups = C) on the ZeroPad2d copy of the channel-last
tensor (the pad kernel counted: the module's own forward launches it) and aten.convolution_backward on that copy with one output
asked for (the data gradient's slice back to the unpadded extent counted), which is what the encoder's training step runs today.
Device time per call from torch.profiler's kernel records: the mean (min - max) of 10 calls after 3 warm-up calls, every kernel a
call launches summed.  Bytes = the operands a call must move (x + y + w, dy + dx + w, x + dy + dw); a device-to-device copy of the
same bytes (it copies half: a copy reads and writes) is timed beside it.  Writes profiles/efficientnet_b0_train_sites.json / .txt.

There is no `step` mode as tools_dev/mobilenet_train_sites.py has one: no front end calls these entries from the training step
(DESIGN.md 6b item 8 d), so there is no setting of `bench.py --train --encoder efficientnet-b0` to compare, and no list of
(op, k, stride) kept on torch either — the table shows none that loses."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# lib/backbone.EfficientNetEncoder.VARIANTS["efficientnet-b0"]: repeat, kernel, stride, expand ratio, input, output
BLOCKS = ((1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80), (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192),
          (1, 3, 1, 6, 192, 320))
LINES = []


def emit(*parts):
    line = " ".join(str(p) for p in parts)
    LINES.append(line)
    print(line, flush=True)


def dw_sites(H=480, W=640):
    """{(Hi, Wi, C, k, stride): [block names]} of the 16 depthwise convolutions, in network order"""
    out = {}
    h, w, idx = H // 2, W // 2, 0
    for repeat, k, stride, expand, inp, oup in BLOCKS:
        for i in range(repeat):
            st, hid = (stride if i == 0 else 1), (inp if i == 0 else oup) * expand
            out.setdefault((h, w, hid, k, st), []).append(f"_blocks.{idx}")
            h, w, idx = h // st, w // st, idx + 1
    return out


def sites(out_path):
    import torch
    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile

    from fastposecnn_amd import _native as nat
    dev = torch.device("cuda:0")
    L = nat.lib()
    B = 8

    def per_call_us(fn, reps=10):
        """device us of each of `reps` calls: the kernel records in launch order, cut into equal runs"""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        evs = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
        evs.sort(key=lambda ev: ev.time_range.start)
        t = [ev.device_time if hasattr(ev, "device_time") else ev.cuda_time for ev in evs]
        k = len(t) // reps
        names = sorted({ev.name.split("(")[0].replace("void ", "")[:48] for ev in evs})
        if k < 1 or k * reps != len(t):      # calls that did not all launch the same kernels: the mean alone
            return [sum(t) / reps] * reps, len(t) / reps, names
        return [sum(t[i * k:(i + 1) * k]) for i in range(reps)], k, names

    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for (Hi, Wi, C, k, s), blocks in dw_sites().items():
        Ho, Wo = Hi // s, Wi // s
        pb, pa = ((k - 1) // 2, (k - 1) // 2) if s == 1 else ((k - 3) // 2, (k - 3) // 2 + 1)      # the static "same" pads
        x = torch.randn((B, C, Hi, Wi), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        gy = torch.randn((B, C, Ho, Wo), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        w = torch.randn((C, 1, k, k), device=dev, generator=g) / k
        y, dx, dw = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w)
        ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        ws = nat.workspace("bench_mb_dw_wgrad", dev, L.fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, k))
        st = nat.stream()
        p = lambda t: t.data_ptr()
        xp = F.pad(x, (pb, pa, pb, pa))      # (the backward of the module's path has this copy saved)
        back = lambda mask: torch.ops.aten.convolution_backward(gy, xp, w, None, [s, s], [0, 0], [1, 1], False, [0, 0], C, mask)
        ops = {
            "fwd": (lambda: nat.check(L.fpc_mbconv_dw(p(x), p(w), p(ones), p(zeros), p(y), B, Hi, Wi, C, k, s, 0, st), "fwd"),
                    lambda: F.conv2d(F.pad(x, (pb, pa, pb, pa)), w, None, s, 0, 1, C), x.numel() + y.numel() + w.numel()),
            "dgrad": (lambda: nat.check(L.fpc_mbconv_dw_dgrad(p(gy), p(w), p(dx), B, Hi, Wi, C, k, s, st), "dgrad"),
                      lambda: back([True, False, False])[0][:, :, pb:pb + Hi, pb:pb + Wi].contiguous(memory_format=torch.channels_last),
                      gy.numel() + dx.numel() + w.numel()),
            "wgrad": (lambda: nat.check(L.fpc_mbconv_dw_wgrad(p(x), p(gy), p(dw), B, Hi, Wi, C, k, s, p(ws), ws.numel(), st), "wgrad"),
                      lambda: back([False, True, False]), x.numel() + gy.numel() + dw.numel()),
        }
        for op, (native, torch_fn, floats) in ops.items():
            nbytes = 4.0 * floats
            n_us, n_k, _ = per_call_us(native)
            t_us, t_k, t_names = per_call_us(torch_fn)
            half = int(nbytes // 8) * 4
            a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
            c_us, _, _ = per_call_us(lambda: b.copy_(a))
            nm, tm, cm = statistics.mean(n_us), statistics.mean(t_us), statistics.mean(c_us)
            spread = max(max(n_us) - min(n_us), max(t_us) - min(t_us))
            verdict = "native faster" if nm < tm - spread else ("torch faster" if nm > tm + spread else "tie")
            rows.append({"site": [Hi, Wi, C, k, s], "blocks": blocks, "op": op, "mbytes": round(nbytes / 1e6, 2),
                         "native_us": [round(nm, 1), round(min(n_us), 1), round(max(n_us), 1)], "native_launches": n_k,
                         "torch_us": [round(tm, 1), round(min(t_us), 1), round(max(t_us), 1)], "torch_launches": t_k, "torch_kernels": t_names,
                         "copy_us": round(cm, 1), "native_gbps": round(nbytes / nm * 1e-3, 1), "torch_gbps": round(nbytes / tm * 1e-3, 1),
                         "copy_gbps": round(nbytes / cm * 1e-3, 1), "verdict": verdict})
            emit(f"{Hi:3d}x{Wi:3d} C{C:4d} k{k} s{s} x{len(blocks)} {op:5s} {nbytes / 1e6:8.2f} MB  native {nm:8.1f} us ({min(n_us):7.1f} - {max(n_us):7.1f}) "
                 f"{rows[-1]['native_gbps']:7.1f} GB/s x{n_k}   torch {tm:8.1f} us ({min(t_us):7.1f} - {max(t_us):7.1f}) {rows[-1]['torch_gbps']:7.1f} GB/s "
                 f"x{t_k}   copy {cm:7.1f} us {rows[-1]['copy_gbps']:7.1f} GB/s   {verdict}")
            del a, b
        del x, xp, gy, y, dx
        torch.cuda.empty_cache()
    for op in ("fwd", "dgrad", "wgrad"):
        for k in (3, 5):
            for s in (1, 2):
                sel = [r for r in rows if r["op"] == op and r["site"][3] == k and r["site"][4] == s]
                n = sum(r["native_us"][0] * len(r["blocks"]) for r in sel)
                t = sum(r["torch_us"][0] * len(r["blocks"]) for r in sel)
                emit(f"per step, {op:5s} k {k} stride {s}: native {n:8.1f} us   torch {t:8.1f} us   ({sum(len(r['blocks']) for r in sel)} sites)")
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame": [480, 640],
           "what": "device us per call (torch.profiler kernel records, every kernel of a call summed): mean, min, max of 10 calls after 3 "
                   "warm-up calls; the copy moves the same bytes (copies half); verdict: the means differ by more than the larger min-max spread",
           "rows": rows}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    sites(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "efficientnet_b0_train_sites.json"))
