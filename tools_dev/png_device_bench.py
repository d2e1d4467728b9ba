"""Device PNG decode against the host decoder, on the frames bench.py's PNG-fed measurement encodes (encode_png_rgb_paeth,
640x480).  Writes profiles/png_device.json.

    python tools_dev/png_device_bench.py            # every step as a child process under its own `timeout`; stops at the first failure
    python tools_dev/png_device_bench.py --step a   # one step, in this process

  a  fpc_png_decode_device alone (compressed bytes already on the device), 32 and 128 files per launch: ms, img/s, and the
     two kernels apart
  b  the host path fpc_png_decode_batch at 1, 2, 4 and 14 threads (no GPU work)
  c  the ResNet34 batch-32 stream of bench.py fed by FrameUploader.upload_png(decode="device") from the submitting thread,
     by upload_png(decode="host", threads=2) and by PngFramePrefetcher with 14 workers (bench.py's own PNG-fed form)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "png_device.json")
LIMITS = {"a": 240, "b": 240, "c": 420}


def frames(n=4):
    import numpy as np
    from bench import encode_png_rgb_paeth
    yy, xx = np.mgrid[0:480, 0:640]
    pngs = []
    for i in range(n):
        img = np.stack([(128 + 100 * np.sin(xx / (23.0 + i)) * np.cos(yy / 31.0)), (xx * 255 / 639 + 20 * i) % 256, (yy * 255 / 479)], -1)
        img = (img + np.random.default_rng(i).integers(0, 24, (480, 640, 3))).clip(0, 255).astype(np.uint8)
        pngs.append(encode_png_rgb_paeth(img))
    return pngs


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def step_a():
    import numpy as np
    import torch
    from fastposecnn_amd import _native as nat
    from fastposecnn_amd.tools import dataset as D
    L, dev = nat.lib(), torch.device("cuda:0")
    pngs = frames()
    want = np.stack([D.imread_png(p, rgb8=True) for p in pngs])
    res = {"png_bytes_per_frame": int(sum(map(len, pngs)) / len(pngs))}
    for n in (32, 128):
        dec = D._DevicePngDecoder(n, 480, 640, dev)
        files = [pngs[i % 4] for i in range(n)]
        used, bpp = dec.pack(files, 3)
        out = torch.empty((n, 480, 640, 3), dtype=torch.uint8, device=dev)
        dec.enqueue(used, bpp, 3, out, 480 * 640 * 3)
        dec.wait()
        assert np.array_equal(out[:4].cpu().numpy(), want) and np.array_equal(out[-4:].cpu().numpy(), want)
        ws = nat.workspace("pngdev", dev, L.fpc_png_decode_device_workspace_bytes(n, 480, 640, bpp))
        args = (nat.ptr(dec.z_dev), used, nat.ptr(dec.desc_dev), n, 480, 640, 3, bpp, nat.ptr(out), 480 * 640 * 3, nat.ptr(dec.status_dev),
                nat.ptr(ws), ws.numel(), nat.stream())
        ms = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nat.check(L.fpc_png_decode_device(*args), "fpc_png_decode_device")
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        for _ in range(5):
            dec.pack(files, 3)
        pack_ms = (time.perf_counter() - t0) / 5 * 1e3
        res["files_%d" % n] = {"ms_per_launch": round(median(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                               "img_per_s": round(n / median(ms) * 1e3, 1), "host_pack_ms": round(pack_ms, 3),
                               "host_pack_img_per_s_one_thread": round(n / pack_ms * 1e3, 1), "compressed_bytes": used}
    return res


def step_b():
    import numpy as np
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    pngs = frames()
    n = 56
    bufs = [np.frombuffer(pngs[i % 4], np.uint8) for i in range(n)]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    out = np.empty((n, 480, 640, 3), np.uint8)
    res = {"files_per_call": n, "cpus_of_this_process": len(os.sched_getaffinity(0))}
    for threads in (1, 2, 4, 14):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            nat.check(L.fpc_png_decode_batch(ptrs, sizes, n, out.ctypes.data, 480, 640, threads), "fpc_png_decode_batch")
            ts.append(time.perf_counter() - t0)
        res["threads_%d" % threads] = {"ms_per_file_per_thread": round(median(ts) / n * threads * 1e3, 3), "img_per_s": round(n / median(ts), 1)}
    return res


def step_c():
    import torch
    import fastposecnn_amd.lib as Lb
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.streaming import FrameStreamer
    from fastposecnn_amd.tools.dataset import FrameUploader, PngFramePrefetcher
    import aggregation_layer as al
    dev, Bq = torch.device("cuda:0"), 32
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING, hp.HV_NUM_OF_HYPOTHESES, hp.ENCODER, hp.ENGINE_TUNE_MODE = False, 1000, "resnet34", 0
    hp.ENGINE_SPLIT_PRECISION = hp.ENGINE_SPLIT_F16 = hp.ENGINE_SPLIT_F16_3P = hp.ENGINE_GRAPH = True
    torch.manual_seed(0)
    model = Lb.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).eval().to(dev)
    x = torch.stack([synth.make_image(i) for i in range(Bq)]).to(dev)
    cat_cpu, _ = synth.make_vote_batch(range(Bq))
    cat = {k: v.to(dev) for k, v in cat_cpu.items()}
    cat["mask"] = al.attach_fg_bits(cat["mask"].to(torch.int64).contiguous())
    streamer = FrameStreamer(model, net_streams=4, post_inline=True, coalesce=1, tune_mode=1)
    depth, AHEAD = len(streamer.models), 2
    streamer.prepare(x, categorical_override=cat, tune_trials=1)
    up = FrameUploader(Bq, 480, 640, device=dev, slots=depth + 2 + AHEAD)
    pngs = frames()
    batch = lambda k: [pngs[(k + j) % 4] for j in range(Bq)]
    pending, uploaded = [], []

    def submit():
        t, ready = uploaded.pop(0)
        pending.append(streamer.submit(t, categorical_override=cat, ready=ready))
        if len(pending) > depth:
            streamer.collect(pending.pop(0))

    def run(feed, nsteps):
        for k in range(nsteps):
            uploaded.append(feed(k))
            if len(uploaded) > AHEAD:
                submit()
        while uploaded:
            submit()
        while pending:
            streamer.collect(pending.pop(0))
        torch.cuda.synchronize()

    def timed(feed, nsteps):
        run(feed, depth + 3)
        t0 = time.perf_counter()
        run(feed, nsteps)
        return round(Bq * nsteps / (time.perf_counter() - t0), 1)

    res = {"workload": "resnet34-FPN + all heads, batch 32, 640x480, %d frames in flight on %d streams, one set of plans" % (depth + 1, depth)}
    res["resident_tensor_img_per_s"] = timed(lambda k: (x, None), 20)
    res["device_decode"] = {"img_per_s": timed(lambda k: up.upload_png(batch(k), decode="device"), 20), "host_threads": 1,
                            "note": "the submitting thread packs; no decode worker"}
    up.check_decoded()
    res["host_decode_2_threads"] = {"img_per_s": timed(lambda k: up.upload_png(batch(k), threads=2), 6), "host_threads": 2}
    n = 20
    pre = iter(PngFramePrefetcher(batch, n + depth + 3, Bq, 480, 640, workers=14))
    res["host_decode_prefetcher"] = {"img_per_s": timed(lambda k: up.upload(next(pre)), n), "host_threads": 14}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps({"a": step_a, "b": step_b, "c": step_c}[args.step]()))
        return
    res = {}
    for step in sorted(LIMITS):
        p = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step],
                           stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            res[step] = {"failed": p.returncode}
            print("step %s failed with status %d: stopping" % (step, p.returncode))
            break
        res[step] = json.loads(lines[-1][7:])
        print(step, json.dumps(res[step]))
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    sys.exit(1 if any("failed" in v for v in res.values()) else 0)


if __name__ == "__main__":
    main()
