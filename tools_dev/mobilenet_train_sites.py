"""The MobileNetV2 encoder's depthwise training kernels against torch's own, and the training step with and without them:
python tools_dev/mobilenet_train_sites.py sites|step [out.json]

sites  every distinct depthwise site of a 640 x 480 frame at the training batch, 8 (csrc/depthwise.hip: k_dw_fwd with the
       identity scale / shift forward, its gradient kernels backward): forward, data gradient and weight gradient each beside
       torch's kernel(s) for the same call in the same process — F.conv2d(groups = C) on the channel-last tensor and
       aten.convolution_backward with one output asked for, which is what the switch-off path (and the parent commit) runs.  Device
       time per call from torch.profiler's kernel records: the mean (min - max) of 10 calls after 3 warm-up calls, every kernel a call
       launches summed.  Bytes = the operands a call must move (x + y + w, dy + dx + w, x + dy + dw); a device-to-device copy of the
       same bytes (it copies half: a copy reads and writes) is timed beside it.  Writes profiles/mobilenet_v2_train_sites.json / .txt.
step   `bench.py --train --encoder mobilenet_v2 --gpus 1` three ways — FPC_TRAIN_NATIVE_MBV2 unset, =1, =1 with FPC_TRAIN_NATIVE_BN=1 —
       alternating, twice, one process each (ms per step: host clock around steps that end in a device synchronise), then one
       steady-state step of each setting under a kernel trace (tools_dev/train_step_stats.py): launches and kernel time.  Writes
       profiles/mobilenet_v2_train_step.txt."""
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
LINES = []


def emit(*parts):
    line = " ".join(str(p) for p in parts)
    LINES.append(line)
    print(line, flush=True)


def dw_sites(H=480, W=640):
    """{(Hi, Wi, C, stride): [block names]} of the 17 depthwise convolutions, in network order"""
    out = {}
    h, w, inp, idx = H // 2, W // 2, 32, 1
    for t, c, n, s in SETTING:
        for i in range(n):
            st, hid = (s if i == 0 else 1), inp * t
            out.setdefault((h, w, hid, st), []).append(f"features.{idx}")
            h, w, inp, idx = h // st, w // st, c, idx + 1
    return out


def sites(out_path):
    import torch
    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile

    from fastposecnn_amd import _native as nat
    from fastposecnn_amd.lib import train_conv
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
    for (Hi, Wi, C, s), blocks in dw_sites().items():
        Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
        x = torch.randn((B, C, Hi, Wi), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        gy = torch.randn((B, C, Ho, Wo), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        w = torch.randn((C, 1, 3, 3), device=dev, generator=g) / 3
        y, dx, dw = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w)
        ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        ws = nat.workspace("bench_dw_wgrad", dev, L.fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C))
        st = nat.stream()
        p = lambda t: t.data_ptr()
        back = lambda mask: torch.ops.aten.convolution_backward(gy, x, w, None, [s, s], [1, 1], [1, 1], False, [0, 0], C, mask)
        ops = {
            "fwd": (lambda: nat.check(L.fpc_dwconv3x3(p(x), p(w), p(ones), p(zeros), p(y), B, Hi, Wi, C, s, 0, st), "fwd"),
                    lambda: F.conv2d(x, w, None, s, 1, 1, C), x.numel() + y.numel() + w.numel()),
            "dgrad": (lambda: nat.check(L.fpc_dwconv3x3_dgrad(p(gy), p(w), p(dx), B, Hi, Wi, C, s, st), "dgrad"),
                      lambda: back([True, False, False]), gy.numel() + dx.numel() + w.numel()),
            "wgrad": (lambda: nat.check(L.fpc_dwconv3x3_wgrad(p(x), p(gy), p(dw), B, Hi, Wi, C, s, p(ws), ws.numel(), st), "wgrad"),
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
            rows.append({"site": [Hi, Wi, C, s], "blocks": blocks, "op": op, "mbytes": round(nbytes / 1e6, 2),
                         "native_us": [round(nm, 1), round(min(n_us), 1), round(max(n_us), 1)], "native_launches": n_k,
                         "torch_us": [round(tm, 1), round(min(t_us), 1), round(max(t_us), 1)], "torch_launches": t_k, "torch_kernels": t_names,
                         "copy_us": round(cm, 1), "native_gbps": round(nbytes / nm * 1e-3, 1), "torch_gbps": round(nbytes / tm * 1e-3, 1),
                         "copy_gbps": round(nbytes / cm * 1e-3, 1), "verdict": verdict,
                         "kept_on_torch": (op, s) in train_conv._DW_KEEP_TORCH})
            emit(f"{Hi:3d}x{Wi:3d} C{C:4d} s{s} x{len(blocks)} {op:5s} {nbytes / 1e6:8.2f} MB  native {nm:8.1f} us ({min(n_us):7.1f} - {max(n_us):7.1f}) "
                 f"{rows[-1]['native_gbps']:7.1f} GB/s x{n_k}   torch {tm:8.1f} us ({min(t_us):7.1f} - {max(t_us):7.1f}) {rows[-1]['torch_gbps']:7.1f} GB/s "
                 f"x{t_k}   copy {cm:7.1f} us {rows[-1]['copy_gbps']:7.1f} GB/s   {verdict}{'  [kept on torch]' if rows[-1]['kept_on_torch'] else ''}")
            del a, b
        del x, gy, y, dx
        torch.cuda.empty_cache()
    for op in ("fwd", "dgrad", "wgrad"):
        for s in (1, 2):
            sel = [r for r in rows if r["op"] == op and r["site"][3] == s]
            n = sum(r["native_us"][0] * len(r["blocks"]) for r in sel)
            t = sum(r["torch_us"][0] * len(r["blocks"]) for r in sel)
            emit(f"per step, {op:5s} stride {s}: native {n:8.1f} us   torch {t:8.1f} us   ({sum(len(r['blocks']) for r in sel)} sites)")
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame": [480, 640],
           "what": "device us per call (torch.profiler kernel records, every kernel of a call summed): mean, min, max of 10 calls after 3 "
                   "warm-up calls; the copy moves the same bytes (copies half); verdict: the means differ by more than the larger min-max spread",
           "rows": rows}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)


SETTINGS = [("off", {}), ("on", {"FPC_TRAIN_NATIVE_MBV2": "1"}), ("on+bn", {"FPC_TRAIN_NATIVE_MBV2": "1", "FPC_TRAIN_NATIVE_BN": "1"})]


def step(out_path):
    base = {k: v for k, v in os.environ.items() if k not in ("FPC_TRAIN_NATIVE_MBV2", "FPC_TRAIN_NATIVE_BN")}
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--train", "--encoder", "mobilenet_v2", "--gpus", "1"]
    emit("mobilenet_v2 training step, B = 8, 640 x 480, one MI355X, one visit, the three settings alternating (off, on, on+bn) x 2:")
    emit("FPC_TRAIN_TRACE=1 [FPC_TRAIN_NATIVE_MBV2=1 [FPC_TRAIN_NATIVE_BN=1]] python bench.py --train --encoder mobilenet_v2 --gpus 1 --steps 20 --warmup 5")
    emit("ms per step, host clock around a step that ends in a device synchronise, 20 steps of one process each:")
    for rep in (1, 2):
        for tag, env in SETTINGS:
            r = subprocess.run(bench + ["--steps", "20", "--warmup", "5"], env={**base, **env, "FPC_TRAIN_TRACE": "1"}, cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                emit(f"{tag} run {rep}: FAILED rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                raise SystemExit(1)
            cum = json.loads([l for l in r.stdout.splitlines() if l.startswith("cumulative ms per step:")][-1].split(":", 1)[1])
            per = [round(b - a, 1) for a, b in zip([0.0] + cum[:-1], cum)]
            emit(f"{tag:6s} run {rep}: median {statistics.median(per):.1f} (min {min(per):.1f} - max {max(per):.1f})   steps: " + " ".join(f"{v:.1f}" for v in per))
    emit("")
    emit("One steady-state step under a kernel trace (--steps 6 --warmup 3, tools_dev/train_step_stats.py), a run of its own per setting:")
    for tag, env in SETTINGS:
        d = tempfile.mkdtemp(prefix="mbv2_trace_" + tag.replace("+", "_") + "_")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"] + bench + ["--steps", "6", "--warmup", "3"],
                           env={**base, **env}, cwd=ROOT, capture_output=True, text=True, timeout=600)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not traces:
            emit(f"{tag}: trace FAILED rc {r.returncode}\n{r.stderr[-2000:]}")
            raise SystemExit(1)
        s = subprocess.run([sys.executable, os.path.join(ROOT, "tools_dev", "train_step_stats.py"), max(traces, key=os.path.getsize), "40"],
                           capture_output=True, text=True, timeout=300)
        emit(f"{tag} ({' '.join(k + '=' + v for k, v in env.items()) or 'both switches unset'}):")
        emit(s.stdout.rstrip() or s.stderr[-2000:])
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "sites"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    if mode == "sites":
        sites(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mobilenet_v2_train_sites.json"))
    elif mode == "step":
        step(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mobilenet_v2_train_step.txt"))
    else:
        raise SystemExit(__doc__)
