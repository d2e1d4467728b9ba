"""Measurement of the evaluate / validate loop's metric stage ("Metrics on the device"): a synthetic
validation loop over the committed fixtures, every batch matched on the device, its metrics taken two ways.
    python tools_dev/eval_epoch.py [--batches 200] [--repeats 5] [--out FILE.json]
host route    DeviceMatches.materialize() (one synchronisation), the six lib/metrics.py accumulators, evaluate.py:238-292's
              per-class loop with every match kept, gtf.calculate_aps / calculate_complex_aps at the end
device route  metrics_device.PoseMetricsDevice.update per batch, aps() at the end
A batch is tests/golden/matching.npz's 7 ground truths x 8 predictions (real masks, real poses) with the predictions' poses
jittered per batch from a seed; both routes see the same batches and their APs are compared before anything is timed.
Per route: ms per batch (host clock around a loop that ends in a synchronise; warm-up first; the two routes alternate
within each repeat), kernel launches and device-to-host copies per batch (torch.profiler's device activity over a few
batches, in a pass of its own) and host synchronisations per batch (torch's sync debug mode, counted from its warnings);
`device_updates_only` leaves out the once-per-epoch aps(), `pose_update_alone` also the matching that both routes share.
Then fpc_confusion_update at 32 x 480 x 640 with HIP events against its algorithmic bytes (16 B per pixel) over 8 TB/s."""
import argparse, json, os, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fastposecnn_amd.lib as L
import metrics as M
import metrics_device as MD

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out")
a = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
dev = torch.device("cuda:0")
gtf, mg = L.gtf, L.mg
KEYS = ("degree_error", "3d_iou", "offset_error")
OPS = {"3d_iou": torch.greater, "degree_error": torch.less, "offset_error": torch.less}
THR = {"3d_iou": torch.cat((torch.tensor([.25, .5]), torch.linspace(0, 1, 50))), "degree_error": torch.cat((torch.tensor([5., 10.]), torch.linspace(0, 60, 50))),
       "offset_error": torch.cat((torch.tensor([5., 10.]), torch.linspace(0, 10, 50)))}         # evaluate.py's table + figure thresholds
CTHR = torch.vstack((torch.tensor([5, 10, 10]), torch.tensor([5, 5, 10])))
CKEY = "degree_error+offset_error"
C = 7

G = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "matching.npz"))
gts = {k[4:]: torch.from_numpy(G[k]).to(dev) for k in G.files if k.startswith("gts_")}
preds0 = {k[6:]: torch.from_numpy(G[k]).to(dev) for k in G.files if k.startswith("preds_")}
gen = torch.Generator().manual_seed(0)


def jittered():
    p = dict(preds0)
    q = preds0["quaternion"].cpu() + 0.15 * torch.randn(preds0["quaternion"].shape, generator=gen)
    p["quaternion"] = (q / q.norm(dim=1, keepdim=True)).to(dev)
    p["T"] = (preds0["T"].cpu() + 0.3 * torch.randn(preds0["T"].shape, generator=gen)).to(dev)
    p["scales"] = (preds0["scales"].cpu() * (0.8 + 0.4 * torch.rand(preds0["scales"].shape, generator=gen))).to(dev)
    return p


batches = [jittered() for _ in range(a.batches)]


def host_route(bs):
    table = M.head_training_metrics()["pose"]
    raw = {k: {} for k in KEYS}
    for p in bs:
        m = mg.batchwise_find_matches_device(p, gts).materialize()
        if m is None:
            continue
        for e in table.values():
            e["F"](m)
        m = {k: v.cpu() for k, v in m.items()}                              # evaluate.py:158: every match is kept on the CPU
        cls = m["class_ids"]
        for c in torch.unique(cls):                                         # :247-286
            i = torch.where(cls == c)[0]
            raw["degree_error"].setdefault(int(c), []).append(gtf.get_quat_distance(m["quaternion"][0][i], m["quaternion"][1][i], m["symmetric_ids"][i]))
            raw["3d_iou"].setdefault(int(c), []).append(gtf.get_3d_ious(m["RT"][0][i], m["RT"][1][i], m["scales"][0][i], m["scales"][1][i]))
            raw["offset_error"].setdefault(int(c), []).append(gtf.from_Ts_get_offset_error(m["T"][0][i], m["T"][1][i]))
    raw = {k: {c: torch.cat(v) for c, v in d.items()} for k, d in raw.items()}
    aps = gtf.calculate_aps(raw, THR, OPS)
    gtf.calculate_complex_aps(raw, {CKEY: CTHR}, OPS)
    torch.cuda.synchronize()
    return aps, {k: float(e["F"].compute()) for k, e in table.items()}


def device_route(bs, pm):
    pm.reset()
    for p in bs:
        pm.update(mg.batchwise_find_matches_device(p, gts))
    aps, caps = pm.aps()
    torch.cuda.synchronize()
    return aps, {k: float(v) for k, v in pm.table().items()}


pm = MD.PoseMetricsDevice(C, THR, {CKEY: CTHR}, device=dev)

# same answers first (the host route's errors here come from the CPU forms: hit counts can differ where an error sits on a threshold)
h_aps, h_tab = host_route(batches)
d_aps, d_tab = device_route(batches, pm)
worst = max(float((h_aps[k][c].cpu() - d_aps[k][c].cpu()).abs().max()) for k in KEYS for c in h_aps[k])
print("largest AP difference between the routes: %.3g (one hit of one class is >= %.3g)" % (worst, 1.0 / (a.batches * 8)))
print("host table  ", h_tab)
print("device table", d_tab)
assert all(set(h_aps[k]) == set(d_aps[k]) for k in KEYS) and worst < 0.02


def ms_per_batch(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3 / a.batches


times = {"host": [], "device": []}
for r in range(a.repeats + 1):                                               # repeat 0 is the warm-up
    th, td = ms_per_batch(lambda: host_route(batches)), ms_per_batch(lambda: device_route(batches, pm))
    if r:
        times["host"].append(th)
        times["device"].append(td)


def census(fn, n):
    """(kernel launches, device-to-host copies, synchronisations) per batch over the first n batches."""
    out = [None, None, None]
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(batches[:n])
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        copies = [e for e in ev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower()]
        d2h = [e for e in copies if "dtoh" in e.name.lower() or "devicetohost" in e.name.lower().replace(" ", "")]
        out[0], out[1] = (len(ev) - len(copies)) / n, len(d2h) / n
    except Exception as e:                                                   # no device tracing in this build: say so
        print("launch census not measured:", repr(e))
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(batches[:n])
        out[2] = sum("synchroniz" in str(x.message).lower() for x in w) / n
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out


def device_updates_only(bs):                                                 # the per-batch part: aps() reads the state back once per epoch
    pm.reset()
    for p in bs:
        pm.update(mg.batchwise_find_matches_device(p, gts))


dms8 = [mg.batchwise_find_matches_device(p, gts) for p in batches[:8]]


def pose_updates_prematched(bs):                                             # the pose part alone: the matching is common to both routes
    for dm in dms8[:len(bs)]:
        pm.update(dm)


res = {"what": "metric stage of the validation loop, %d batches of 7 x 8 instances, MI355X" % a.batches, "repeats": a.repeats}
for name, fn in (("host", host_route), ("device", lambda bs: device_route(bs, pm)), ("device_updates_only", device_updates_only),
                 ("pose_update_alone", pose_updates_prematched)):
    k, c, s = census(fn, 8)
    t = times.get(name)
    res[name] = {"launches_per_batch": k, "d2h_copies_per_batch": c, "host_syncs_per_batch": s}
    if t:
        res[name].update(ms_per_batch_median=round(float(np.median(t)), 4), ms_per_batch_min=round(min(t), 4), ms_per_batch_max=round(max(t), 4))
    print(name, res[name])

# the confusion kernel at the issue's size
B, H, W = 32, 480, 640
g2 = torch.Generator().manual_seed(1)
gt_mask = torch.randint(0, C, (B, H // 8, W // 8), generator=g2).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous().to(dev)     # 8 x 8 blobs
flip = torch.rand((B, H, W), generator=g2) < 0.1
pred_mask = torch.where(flip, torch.randint(0, C, (B, H, W), generator=g2), gt_mask.cpu()).to(dev)
noise = torch.randint(0, C, (B, H, W), generator=g2).to(dev)
mm = MD.MaskMetricsDevice(C, device=dev)
res["confusion"] = {}
for name, (pm_, gm_) in (("blobs_10pct_wrong", (pred_mask, gt_mask)), ("uniform_random_labels", (noise, gt_mask)), ("one_class", (torch.zeros_like(noise), torch.zeros_like(noise)))):
    mm.reset()
    mm.update(pm_, gm_)
    want = torch.bincount((C * gm_ + pm_).reshape(-1), minlength=C * C)
    assert torch.equal(mm.confusion().reshape(-1), want)
    us = []
    for r in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            mm.update(pm_, gm_)
        e1.record()
        torch.cuda.synchronize()
        if r:
            us.append(e0.elapsed_time(e1) / 50 * 1e3)
    nbytes = 16 * B * H * W
    floor_us = nbytes / 8e12 * 1e6
    res["confusion"][name] = {"us_median": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "bytes": nbytes,
                              "hbm_floor_us": round(floor_us, 2), "fraction_of_8TBps": round(floor_us / float(np.median(us)), 4)}
    print("confusion", name, res["confusion"][name])
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
