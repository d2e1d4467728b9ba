"""What feeding the ground truth costs: 32 frames of 640 x 480 with 6 elliptical instances each (config 3), id planes and
side-file dicts synthesised in memory (the ellipses of fastposecnn_amd/synth.py, RGBA id planes as the CAMERA set's mask
files decode).

  (a) host path: the ground-truth body of NOCSDataset.__getitem__ on the in-memory id plane (float mask, the two table
      sweeps, generate_agg_data, class mask) per frame, then my_collate_fn(..., device).  The image and depth keys are left
      out on both sides: they are the colour path's.
  (b) GroundTruthUploader.upload for each mask_dtype, gt_from_side_file included: synchronised after every batch, and
      pipelined through the slots (one synchronise at the end).
  (c) fpc_gt_build alone on resident inputs: device events around back-to-back launches (the entry's memset of the
      counts included), and its share of the HBM rate on the bytes it writes, n H W elem + 8 B H W.

    python tools_dev/gt_feed_bench.py [--out profiles/gt_feed.json]

Prints one JSON line.  Needs the GPU: there is no host substitute for (b) and (c)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fastposecnn_amd import _native as nat, synth  # noqa: E402
from fastposecnn_amd.tools import dataset as D  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12      # bytes/s: float4 copy as measured on the MI355X, and the data sheet's figure


def synth_frame(frame, K, H, W):
    """-> (RGBA id plane uint8 [H,W,4], side-file dict as json.load returns it)."""
    g = torch.Generator().manual_seed(1000 + frame)
    r = np.random.default_rng(1000 + frame)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    plane = r.integers(0, 256, (H, W, 4)).astype(np.uint8)
    plane[..., 0] = 255                                                        # the files' background
    side = {"instance_dict": {}, "scales": [], "quaternions": [], "RTs": [], "norm_factors": []}
    for k, (ex, ey, rx, ry) in enumerate(synth._place_ellipses(K, H, W, g, 30.0, 110.0)):
        plane[..., 0][((xx - ex) / rx) ** 2 + ((yy - ey) / ry) ** 2 <= 1.0] = k + 1
        q = r.normal(size=4)
        q /= np.linalg.norm(q)
        a, b, c, d = q
        pose = np.eye(4)
        pose[:3, :3] = [[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                        [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                        [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]]
        pose[:3, 3] = [r.uniform(-0.2, 0.2), r.uniform(-0.2, 0.2), r.uniform(0.6, 1.2)]      # in front of the camera
        side["instance_dict"][str(k + 1)] = 1 + k % 6
        side["scales"].append(r.uniform(0.1, 0.5, 3).tolist())
        side["quaternions"].append(q.tolist())
        side["RTs"].append(np.linalg.inv(pose).tolist())
        side["norm_factors"].append(float(r.uniform(0.3, 1.0)))
    return plane, side


def host_item(ds, plane, side):
    """NOCSDataset.__getitem__'s ground-truth lines on a decoded mask (tools/dataset.py)."""
    mask = plane[:, :, 0].astype('float')
    mask[mask == 255] = 0
    good = ds.wanted_instances(side)
    id_of = np.zeros(256, dtype=mask.dtype)
    class_of = np.zeros(256, dtype=mask.dtype)
    for inst_id, c in good['instance_dict'].items():
        id_of[inst_id] = inst_id
        class_of[inst_id] = c
    pixel_ids = mask.astype(np.intp)
    agg_data = ds.generate_agg_data(id_of[pixel_ids], good)
    if (agg_data['z'] <= 0).any():
        return None
    return {'mask': class_of[pixel_ids].astype('long'), 'agg_data': agg_data}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--instances", type=int, default=6)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_feed_bench: no GPU")
    dev = torch.device("cuda:0")
    B, K, H, W = a.frames, a.instances, a.height, a.width
    with tempfile.TemporaryDirectory() as empty:
        ds = D.CAMERADataset(empty)                                            # no frame on disk: its methods are what is wanted
    frames = [synth_frame(f, K, H, W) for f in range(B)]
    planes = np.stack([p for p, _ in frames])
    sides = [s for _, s in frames]
    n = B * K
    res = {"frames": B, "instances": n, "height": H, "width": W, "device": torch.cuda.get_device_name(0)}

    def host_batch():
        batch = D.my_collate_fn([host_item(ds, p, s) for p, s in frames], dev)
        torch.cuda.synchronize()
        return batch

    want = host_batch()
    t = timed(host_batch, a.host_reps, 1)
    res["a_host_batches_per_s"] = 1.0 / t
    res["a_host_bytes_over_the_bus"] = int(sum(v.numel() * v.element_size() for v in want["agg_data"].values())
                                           + want["mask"].numel() * 8)

    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32"), (torch.uint8, "u8")):
        up = D.GroundTruthUploader(B, H, W, 4, device=dev, slots=2, max_instances=256, mask_dtype=dtype)
        state = {}

        def one(sync):
            got, ready = up.upload(planes, [ds.gt_from_side_file(s) for s in sides])
            if sync:
                ready.synchronize()
            state["got"] = got

        one(True)
        got = state["got"]
        assert torch.equal(got["mask"], want["mask"])                          # the same batch as the host path's
        for key, w in want["agg_data"].items():
            g = got["agg_data"][key]
            assert torch.equal(g.to(w.dtype), w), key
        D.GroundTruthUploader.check(got)
        res["b_upload_%s_batches_per_s" % name] = 1.0 / timed(lambda: one(True), a.reps, 3)
        res["b_upload_%s_pipelined_batches_per_s" % name] = 1.0 / timed(lambda: one(False), a.reps, 3)
        del up, got, state
        torch.cuda.empty_cache()
    res["b_upload_bytes_over_the_bus"] = int(planes.nbytes)

    # (c) the kernel alone
    items = [ds.gt_from_side_file(s) for s in sides]
    row_of, class_of, first_row, n = D.gt_tables(items)
    t_ids, t_row, t_cls, t_first = (torch.from_numpy(x).to(dev) for x in (planes, row_of, class_of, first_row))
    cm = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    L = nat.lib()
    for dtype, name, elem in ((torch.float64, "f64", 8), (torch.float32, "f32", 4), (torch.uint8, "u8", 1)):
        inst = torch.empty((n, H, W), dtype=dtype, device=dev)

        def launch():
            nat.check(L.fpc_gt_build(nat.ptr(t_ids), 4, H * W * 4, B, H, W, nat.ptr(t_row), nat.ptr(t_cls), nat.ptr(t_first), n,
                                     nat.ptr(cm), nat.ptr(inst), elem, nat.ptr(count), nat.stream()), "fpc_gt_build")

        for _ in range(5):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 100
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        e1.synchronize()
        sec = e0.elapsed_time(e1) * 1e-3 / reps
        written = n * H * W * elem + 8 * B * H * W
        res["c_kernel_%s_us" % name] = sec * 1e6
        res["c_kernel_%s_bytes_written" % name] = int(written)
        res["c_kernel_%s_tb_per_s" % name] = written / sec / 1e12
        res["c_kernel_%s_share_of_measured_hbm" % name] = written / sec / HBM_MEASURED
        res["c_kernel_%s_share_of_spec_hbm" % name] = written / sec / HBM_SPEC
        del inst
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
