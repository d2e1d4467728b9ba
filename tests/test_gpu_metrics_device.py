"""The metric accumulators on the device (csrc/pose_metrics.hip, csrc/confusion.hip, lib/metrics_device.py) against the host
route they stand in for: the six lib/metrics.py classes fed the materialised match, evaluate.py:238-292's per-class loop
with gtf.calculate_aps / calculate_complex_aps, and np.bincount for the confusion matrix.  Bars: counts exact; running
means rtol 1e-5 (test_eval_losses.py's bar for f32 means: the host takes them in f32, the device sums in f64); raw errors at
_check_eval's bars (1e-4; IoU rtol 2e-4 / atol 1e-7).  Hit counts are exact on the condition, asserted on the host's values,
that no error lies within 1e-4 relative of a threshold: the seeds are chosen so that it holds."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

GT_CLS = [2, 1, 1, 3, 1, 5, 1]                          # the crafted 7 x 8 assignment of test_gpu_match_loss.py
PRED_CLS = [1, 1, 2, 1, 4, 3, 2, 5]
NAN = float("nan")
IOU = [[.9, .9, .3, .9, .9, .9, .3, .9],            # tie inside class 2 -> p2; larger values of other classes ignored
       [.5, .5, .9, .2, .9, .9, .9, .9],            # tie p0 / p1 -> p0
       [.6, .1, .9, .0, .9, .9, .9, .9],            # p0 again (one prediction, two ground truths)
       [.9, .9, .9, .9, .9, .0, .9, .9],            # its class's only prediction has IoU 0 -> unmatched
       [.7, NAN, .9, .8, .9, .9, .9, .9],           # NaN inside its class -> unmatched
       [NAN, NAN, NAN, NAN, NAN, NAN, NAN, .25],    # NaN only in other classes -> p7
       [.0, .0, .9, .4, .9, .9, .9, .9]]            # p3
C = 7
SEEDS = (43, 55, 64)                                    # clear of every threshold by 5e-4 relative on the CPU forms; symmetric ids 0, 1 and 2 in each
KEYS = ("degree_error", "3d_iou", "offset_error")
TABLE_THR = {"degree_error": [5., 10.], "3d_iou": [.25, .5], "offset_error": [5., 10.]}                      # evaluate.py:220-224
FIGURE = {"degree_error": (0, 60), "3d_iou": (0, 1), "offset_error": (0, 10)}                                # :213-217, 50 points
CTHR = [[5, 10, 10], [5, 5, 10]]                                                                             # :226-228
CKEY = "degree_error+offset_error"
OPS = {"degree_error": torch.less, "3d_iou": torch.greater, "offset_error": torch.less}


def full_thresholds():
    return {k: torch.cat((torch.tensor(TABLE_THR[k]), torch.linspace(*FIGURE[k], 50))) for k in KEYS}


def table_thresholds():
    return {k: torch.tensor(TABLE_THR[k]) for k in KEYS}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mods(dev):
    import fastposecnn_amd.lib  # noqa: F401
    from fastposecnn_amd import _native
    _native.lib()
    import gpu_tensor_funcs as gtf
    import matching as mg
    import metrics as M
    import metrics_device as MD
    return gtf, mg, M, MD


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene_np(cls, seed, sym=None):
    """An AggData-like dict of len(cls) instances around one common pose, so that any two boxes overlap: unit quaternions,
    RT = [[R, t], [0 0 0 1]] with R a rotation (a proper rigid transform), 4 x 6 instance masks."""
    r = np.random.default_rng(seed)
    n = len(cls)
    base = np.array([0.8, 0.2, -0.4, 0.4])
    q = base + 0.25 * r.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    qr = base + 0.02 * r.normal(size=(n, 4))
    qr /= np.linalg.norm(qr, axis=1, keepdims=True)
    t = np.array([0.3, -0.2, 1.5]) + 0.1 * r.normal(size=(n, 3))
    RT = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        RT[i, :3, :3], RT[i, :3, 3] = _rot(qr[i]), t[i]
    return {"class_ids": np.asarray(cls, np.int64), "sample_ids": r.integers(0, 3, n).astype(np.int64),
            "symmetric_ids": (r.integers(0, 3, n) if sym is None else np.full(n, sym)).astype(np.int64),
            "instance_masks": np.zeros((n, 4, 6), np.float32), "quaternion": q.astype(np.float32),
            "scales": (1.5 + 0.5 * r.random((n, 3))).astype(np.float32), "xy": (3 * r.normal(size=(n, 2))).astype(np.float32),
            "z": (500 + 1000 * r.random((n, 1))).astype(np.float32), "R": RT[:, :3, :3].astype(np.float32),
            "T": (0.5 * r.normal(size=(n, 3))).astype(np.float32), "RT": RT.astype(np.float32)}


def scene(cls, seed, dev, sym=None):
    return {k: torch.from_numpy(v).to(dev) for k, v in scene_np(cls, seed, sym).items()}


def crafted_pair(seed, dev):
    return scene(GT_CLS, seed, dev), scene(PRED_CLS, seed + 100, dev)


@pytest.fixture
def crafted_iou(mods, dev, monkeypatch):
    iou = torch.tensor(IOU, dtype=torch.float32, device=dev)
    monkeypatch.setattr(mods[0], "batchwise_get_2d_iou", lambda a, b: iou)


def identity_matches(mg, gts, preds, dev):
    """Ground truth i matched to prediction i, in index order, as fpc_match_assign would leave it."""
    n = gts["class_ids"].shape[0]
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    return mg.DeviceMatches(preds, gts, idx.clone(), idx.clone(), torch.tensor([n], dtype=torch.int32, device=dev))


class HostRoute:
    """The parent's route over a sequence of materialised matches."""

    def __init__(self, gtf, M, with_offset_error=True):
        self.gtf = gtf
        self.table = M.head_training_metrics()["pose"]
        if not with_offset_error:
            del self.table["offset_error"]              # torch.inverse raises on a singular RT
        self.out = {}
        self.raw = {k: {} for k in KEYS}                # evaluate.py's lists: degree through get_quat_distance
        self.pairs = {k: [] for k in KEYS + ("cls",)}   # every pair's three errors in pair order

    def update(self, m):
        gtf = self.gtf
        if m is None:
            return
        self.out = {k: e["F"](m) for k, e in self.table.items()}
        cls = m["class_ids"]
        for c in torch.unique(cls):
            i = torch.where(cls == c)[0]
            vals = (gtf.get_quat_distance(m["quaternion"][0][i], m["quaternion"][1][i], m["symmetric_ids"][i]),
                    gtf.get_3d_ious(m["RT"][0][i], m["RT"][1][i], m["scales"][0][i], m["scales"][1][i]),
                    gtf.from_Ts_get_offset_error(m["T"][0][i], m["T"][1][i]))
            for k, v in zip(KEYS, vals):
                self.raw[k].setdefault(int(c), []).append(v)
        deg, iou, off = gtf._pose_errors(m["quaternion"][0], m["quaternion"][1], m["symmetric_ids"], m["RT"][0], m["RT"][1],
                                         m["scales"][0], m["scales"][1], m["T"][0], m["T"][1])
        for k, v in zip(KEYS + ("cls",), (deg, iou, off, cls)):
            self.pairs[k].append(v)

    def aps(self, thr, dev):
        raw = {k: {c: torch.cat(v) for c, v in d.items()} for k, d in self.raw.items()}
        return self.gtf.calculate_aps(raw, {k: v.to(dev) for k, v in thr.items()}, OPS)

    def complex_aps(self, dev):
        p = {k: torch.cat(v) for k, v in self.pairs.items()}
        raw = {k: {int(c): torch.nan_to_num(p[k][p["cls"] == c].double(), nan=1e9) for c in torch.unique(p["cls"])} for k in KEYS}
        return self.gtf.calculate_complex_aps(raw, {CKEY: torch.tensor(CTHR).to(dev)}, OPS)

    def assert_clear_of(self, thr):
        """The condition of the exact hit counts: no host error within 1e-4 relative of a threshold."""
        for k in KEYS:
            v = torch.cat(self.pairs[k]).double().cpu().numpy()
            v = v[~np.isnan(v)]
            t = thr[k].double().numpy()
            if k != "3d_iou":
                t = np.concatenate((t, np.asarray(CTHR[0 if k == "degree_error" else 1], np.float64)))
            gap = np.abs(v[:, None] - t[None, :]) - 1e-4 * np.abs(t[None, :])
            assert (gap > 0).all(), (k, v[np.where(gap <= 0)[0]], t[np.where(gap <= 0)[1]])


def assert_same_aps(got, want):
    assert set(got) == set(want)
    for k in want:
        assert set(got[k]) == set(want[k]), (k, set(got[k]), set(want[k]))
        for c, v in want[k].items():
            assert got[k][c].dtype == v.dtype and torch.equal(got[k][c], v), (k, c, got[k][c], v)


def assert_same_table(pm, host, n_updates=None):
    got = pm.table()
    s = pm.state.cpu()
    for name, w in (("degree_error_AP_5", 4), ("iou_3d_mAP_0.25", 6), ("offset_error_AP_5cm", 8)):
        F = host.table[name]["F"]
        assert int(s[w]) == int(F.correct) and int(s[w + 1]) == int(F.total), (name, s[w:w + 2].tolist(), int(F.correct), int(F.total))
        # the counts are exact; the host's f32 percentage divides a device scalar by a host one (torch multiplies by the
        # reciprocal there), so it may sit one or two f32 roundings (2^-23 each) from the plain quotient
        np.testing.assert_allclose(float(got[name]), float(host.out[name]), rtol=4 * 2.0 ** -23, err_msg=name)
    for name in ("degree_error", "iou_3d_accuracy", "offset_error"):
        if name in host.table:
            print(name, float(got[name]), float(host.out[name]))
            np.testing.assert_allclose(float(got[name]), float(host.out[name]), rtol=1e-5, err_msg=name)
    if n_updates is not None:
        assert int(s[0]) == n_updates


def run_crafted(mods, dev, thr, keep_raw=0, empty_between=False):
    gtf, mg, M, MD = mods
    pm = MD.PoseMetricsDevice(C, thr, {CKEY: CTHR}, keep_raw=keep_raw, device=dev)
    host = HostRoute(gtf, M)
    for n, seed in enumerate(SEEDS):
        gts, preds = crafted_pair(seed, dev)
        dm = mg.batchwise_find_matches_device(preds, gts)
        pm.update(dm)
        host.update(dm.materialize())
        if empty_between and n == 0:
            yield pm
    yield pm, host


def test_against_the_host_route(mods, dev, crafted_iou):
    gtf, mg, M, MD = mods
    thr = full_thresholds()
    before = dict(MD.counters)
    (pm, host), = run_crafted(mods, dev, thr, keep_raw=64)
    assert MD.counters["device"] == before["device"] + 3 and MD.counters["fallback"] == before["fallback"]
    host.assert_clear_of(thr)
    assert_same_table(pm, host, n_updates=3)
    aps, caps = pm.aps()
    assert_same_aps(aps, host.aps(thr, dev))
    assert_same_aps(caps, host.complex_aps(dev))
    assert set(aps["degree_error"]) == {1, 2, 5, "mean"}
    assert int(pm.skipped()) == 0 and int(pm.overflow()) == 0 and int(pm.state[2]) == 15
    raw = pm.raw()
    p = {k: torch.cat(v) for k, v in host.pairs.items()}
    identical = True
    for k, tol in (("degree_error", dict(rtol=1e-4, atol=1e-4)), ("3d_iou", dict(rtol=2e-4, atol=1e-7)), ("offset_error", dict(rtol=1e-4, atol=1e-4))):
        assert set(raw[k]) == {1, 2, 5}
        for c, v in raw[k].items():
            want = p[k][p["cls"] == c]
            assert v.dtype == want.dtype
            np.testing.assert_allclose(v.cpu().numpy(), want.cpu().numpy(), err_msg=f"{k} {c}", **tol)
            identical = identical and torch.equal(v, want)
    print("raw log bit-identical to fpc_pose_errors:", identical)


def test_golden_pairs_as_one_update(mods, dev):
    """tests/golden/eval_losses.npz: the 11 pairs, identity-matched.  The golden's raw IoU is in percent and its class-1
    degree list starts with an injected NaN (oracle/gen_golden.py): here pair 0's predicted quaternion is NaN, a plain pair."""
    gtf, mg, M, MD = mods
    G = load_golden("eval_losses.npz")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = G["q0"].shape[0]
    assert G["sym"][0] == 0 and G["cls"][0] == 1
    q1 = G["q1"].copy()
    q1[0] = NAN
    base = {"class_ids": t(G["cls"]), "instance_masks": torch.zeros((n, 4, 6), device=dev)}
    gts = dict(base, symmetric_ids=t(G["sym"]), quaternion=t(G["q0"]), RT=t(G["RT0"]), scales=t(G["s0"]), T=t(G["T0"]))
    preds = dict(base, quaternion=t(q1), RT=t(G["RT1"]), scales=t(G["s1"]), T=t(G["T1"]))
    thr = {"degree_error": torch.tensor([5., 10., 30., 60.]), "3d_iou": torch.tensor([1., 10., 25., 50.]) / 100,
           "offset_error": torch.tensor([5., 10., 50., 200.])}
    pm = MD.PoseMetricsDevice(7, thr, {CKEY: [[5, 10, 60], [5, 50, 200]]}, keep_raw=16, device=dev)
    pm.update(identity_matches(mg, gts, preds, dev))
    aps, caps = pm.aps()
    classes = set(int(c) for c in np.unique(G["cls"])) | {"mean"}
    for k in KEYS:
        assert set(aps[k]) == classes
        for c, v in aps[k].items():
            np.testing.assert_allclose(v.cpu().numpy(), G[f"aps_{k}_{c}"], rtol=1e-6, err_msg=f"{k} {c}")
    assert set(caps[CKEY]) == classes
    for c, v in caps[CKEY].items():
        np.testing.assert_allclose(v.cpu().numpy(), G[f"caps_{c}"], rtol=1e-6, err_msg=f"complex {c}")
    raw = pm.raw()
    for c in np.unique(G["cls"]):
        c = int(c)
        np.testing.assert_allclose(raw["degree_error"][c].cpu().numpy(), G[f"raw_degree_error_{c}"], rtol=1e-4, atol=1e-4, equal_nan=True)
        np.testing.assert_allclose(raw["3d_iou"][c].cpu().numpy() * np.float32(100), G[f"raw_3d_iou_{c}"], rtol=2e-4, atol=1e-5)
        np.testing.assert_allclose(raw["offset_error"][c].cpu().numpy(), G[f"raw_offset_error_{c}"], rtol=1e-4, atol=1e-4)


def test_strict_comparisons(mods, dev):
    gtf, mg, M, MD = mods
    gts, preds = scene([1], 5, dev, sym=0), scene([1], 5, dev, sym=0)             # the same instance twice: identical boxes
    gts["T"] = torch.tensor([[0.5, 0.75, 1.0]], device=dev)
    preds["T"] = torch.tensor([[0.125, 0.25, 1.0]], device=dev)                    # T1 - T2 = (0.375, 0.5, 0): |.| = 0.625 exactly
    assert gtf.from_Ts_get_offset_error(gts["T"], preds["T"]).tolist() == [6.25]
    assert gtf.get_3d_ious(gts["RT"], preds["RT"], gts["scales"], preds["scales"]).tolist() == [1.0]
    assert gtf.get_quat_distance(gts["quaternion"], preds["quaternion"], gts["symmetric_ids"]).tolist() == [0.0]
    thr = {"degree_error": torch.tensor([0., 1.]), "3d_iou": torch.tensor([1., 0.5]), "offset_error": torch.tensor([6.25, 6.5])}
    pm = MD.PoseMetricsDevice(3, thr, {CKEY: [[0, 1, 1], [7, 6.25, 7]]}, table_thresholds=(0, 1.0, 6.25), device=dev)
    pm.update(identity_matches(mg, gts, preds, dev))
    aps, caps = pm.aps()
    for k in KEYS:
        assert aps[k][1].tolist() == [0.0, 1.0], k                                # equal to the threshold is not a hit
    assert caps[CKEY][1].tolist() == [0.0, 0.0, 1.0]
    assert pm.state[4:10].tolist() == [0, 1, 0, 1, 0, 1]


def test_nan_rules(mods, dev):
    """Pair 0: a NaN quaternion (degree error NaN); pair 1: a singular RT (IoU NaN)."""
    gtf, mg, M, MD = mods
    gts, preds = scene([1, 1], 21, dev, sym=0), scene([1, 1], 22, dev, sym=0)
    preds["quaternion"][0] = NAN
    preds["RT"][1] = 0.0
    thr = table_thresholds()
    pm = MD.PoseMetricsDevice(3, thr, {CKEY: CTHR}, device=dev)
    dm = identity_matches(mg, gts, preds, dev)
    pm.update(dm)
    host = HostRoute(gtf, M, with_offset_error=False)
    host.update(dm.materialize())
    deg, iou, off = (torch.cat(host.pairs[k]).cpu().numpy() for k in KEYS)
    assert np.isnan(deg).tolist() == [True, False] and np.isnan(iou).tolist() == [False, True] and not np.isnan(off).any()
    host.assert_clear_of(thr)
    L, s = pm.layout, pm.state.cpu()
    assert [int(s[L.samples(1, m) + j]) for m in range(3) for j in range(2)] == [1, 1, 1, 1, 2, 0]      # valid, NaN per metric
    assert_same_table(pm, host)                                          # Iou3dAP.total keeps the NaN pair, DegreeErrorMeanAP's drops it
    assert s[5] == 1 and s[7] == 2 and s[9] == 2
    aps, caps = pm.aps()
    assert_same_aps(aps, host.aps(thr, dev))                             # calculate_aps drops the NaN from the denominator
    assert aps["degree_error"][1].tolist() == [float(deg[1] < 5), float(deg[1] < 10)]
    assert aps["3d_iou"][1].tolist() == [float(iou[0] > .25), float(iou[0] > .5)]
    assert_same_aps(caps, host.complex_aps(dev))
    assert np.isnan(float(pm.table()["iou_3d_accuracy"])) and np.isnan(float(pm.table()["offset_error"]))


def test_nothing_matched_leaves_the_state(mods, dev, crafted_iou, monkeypatch):
    gtf, mg, M, MD = mods
    thr = table_thresholds()
    runs = run_crafted(mods, dev, thr, keep_raw=8, empty_between=True)
    pm = next(runs)                                                      # one real update so far
    before = pm.state.clone()
    raw_before = [b.clone() for b in pm._raw]
    zero = torch.zeros((7, 8), device=dev)
    monkeypatch.setattr(gtf, "batchwise_get_2d_iou", lambda a, b: zero)
    dm = mg.batchwise_find_matches_device(*reversed(crafted_pair(99, dev)))
    pm.update(dm)
    assert dm.count.tolist() == [0]
    assert torch.equal(pm.state, before) and all(torch.equal(a, b) for a, b in zip(pm._raw, raw_before))
    iou = torch.tensor(IOU, dtype=torch.float32, device=dev)
    monkeypatch.setattr(gtf, "batchwise_get_2d_iou", lambda a, b: iou)
    pm, host = next(runs)
    (pm2, _), = run_crafted(mods, dev, thr, keep_raw=8)
    assert torch.equal(pm.state, pm2.state)
    assert_same_table(pm, host, n_updates=3)
    fresh = MD.PoseMetricsDevice(C, thr, device=dev)
    fresh.update(dm)
    assert not fresh.state.any()


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("sym", [0, 1])
def test_all_plain_or_all_symmetric(mods, dev, sym, n):
    """One pair, and one pair more than a wave of them (more than one pass of the kernel's waves)."""
    gtf, mg, M, MD = mods
    cls = [1 + i % 6 for i in range(n)]
    gts, preds = scene(cls, 31 + n, dev, sym=sym), scene(cls, 32 + n, dev, sym=sym)
    thr = table_thresholds()
    pm = MD.PoseMetricsDevice(C, thr, {CKEY: CTHR}, device=dev)
    host = HostRoute(gtf, M)
    dm = identity_matches(mg, gts, preds, dev)
    pm.update(dm)
    host.update(dm.materialize())
    host.assert_clear_of(thr)
    assert_same_table(pm, host, n_updates=1)
    aps, caps = pm.aps()
    assert_same_aps(aps, host.aps(thr, dev))
    assert_same_aps(caps, host.complex_aps(dev))
    assert int(pm.state[7]) == n


def test_raw_log_overflow(mods, dev):
    gtf, mg, M, MD = mods
    thr = table_thresholds()
    pm = MD.PoseMetricsDevice(3, thr, keep_raw=5, device=dev)
    want = []
    for seed in (41, 42):
        gts, preds = scene([1] * 4, seed, dev), scene([1] * 4, seed + 100, dev)
        pm.update(identity_matches(mg, gts, preds, dev))
        want.append(gtf.from_Ts_get_offset_error(gts["T"], preds["T"]))
    raw = pm.raw()
    assert set(raw["offset_error"]) == {1} and raw["degree_error"][1].shape[0] == raw["3d_iou"][1].shape[0] == 5
    np.testing.assert_allclose(raw["offset_error"][1].cpu().numpy(), torch.cat(want)[:5].cpu().numpy(), rtol=1e-6)      # the first five, in order
    assert int(pm.overflow()) == 3 and int(pm.state[2]) == 8
    L = pm.layout
    assert [int(pm.state[L.samples(1, m)] + pm.state[L.samples(1, m) + 1]) for m in range(3)] == [8, 8, 8]
    assert int(pm.state[7]) == 8 and int(pm.state[0]) == 2


def test_class_ids_out_of_range_are_skipped(mods, dev):
    gtf, mg, M, MD = mods
    gts, preds = scene([0, 1, 3, -2, 2], 51, dev), scene([0, 1, 3, -2, 2], 52, dev)
    pm = MD.PoseMetricsDevice(3, table_thresholds(), {CKEY: CTHR}, keep_raw=8, device=dev)
    pm.update(identity_matches(mg, gts, preds, dev))
    L, s = pm.layout, pm.state.cpu()
    assert int(pm.skipped()) == 3 and int(s[7]) == 5                      # classes 0, 3, -2: in table() and the log only
    assert [int(s[L.samples(c, 0)] + s[L.samples(c, 0) + 1]) for c in range(3)] == [0, 1, 1]
    assert sorted(pm.raw()["offset_error"]) == [-2, 0, 1, 2, 3]


def _confusion_want(pred, gt, Cn):
    p, g = pred.reshape(-1).astype(np.int64), gt.reshape(-1).astype(np.int64)
    ok = (p >= 0) & (p < Cn) & (g >= 0) & (g < Cn)
    return np.bincount(Cn * g[ok] + p[ok], minlength=Cn * Cn), int((~ok).sum())


@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (3, 5, 7, 7), (1, 3, 67, 7), (2, 480, 640, 7), (1, 8, 1031, 32)])
def test_confusion_random_planes(mods, dev, shape):
    MD = mods[3]
    B, H, W, Cn = shape
    r = np.random.default_rng(B * H * W)
    pred, gt = r.integers(0, Cn, (B, H, W)), r.integers(0, Cn, (B, H, W))
    mm = MD.MaskMetricsDevice(Cn, device=dev)
    mm.update(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))
    want, skipped = _confusion_want(pred, gt, Cn)
    assert np.array_equal(mm.confusion().cpu().numpy().reshape(-1), want) and int(mm.skipped()) == skipped == 0
    # planes that start 8 bytes off a 16-byte boundary take the scalar-load form
    fp, fg = torch.from_numpy(pred).to(dev).reshape(-1)[1:], torch.from_numpy(gt).to(dev).reshape(-1)[1:]
    assert fp.data_ptr() % 16 == 8 or fp.numel() == 0
    mm.reset()
    if fp.numel():
        mm.update(fp, fg)
        want, _ = _confusion_want(pred.reshape(-1)[1:], gt.reshape(-1)[1:], Cn)
        assert np.array_equal(mm.confusion().cpu().numpy().reshape(-1), want)


def test_confusion_contention_ignore_labels_and_no_wrap(mods, dev):
    MD = mods[3]
    Cn = 7
    mm = MD.MaskMetricsDevice(Cn, device=dev)
    mm.state[3 * Cn + 3] = 2 ** 31 - 3                                   # the global state is 64-bit: no wrap at 2^31 or 2^32
    ones = torch.full((1, 480, 640), 3, dtype=torch.int64, device=dev)   # every pixel on one counter
    mm.update(ones, ones)
    want = np.zeros(Cn * Cn, np.int64)
    want[3 * Cn + 3] = 2 ** 31 - 3 + 480 * 640
    assert np.array_equal(mm.confusion().cpu().numpy().reshape(-1), want) and int(mm.skipped()) == 0
    r = np.random.default_rng(8)
    pred, gt = r.integers(0, Cn, (2, 480, 640)), r.integers(0, Cn, (2, 480, 640))
    flat = gt.reshape(-1)
    at = r.choice(flat.size, 1500, replace=False)
    flat[at[:1000]], flat[at[1000:]] = 255, -1                           # ignore labels in known numbers
    pred.reshape(-1)[at[:10]] = -1                                       # both out of range: still one pixel
    pred.reshape(-1)[r.choice(np.setdiff1d(np.arange(flat.size), at), 7, replace=False)] = Cn      # a prediction one past the classes
    mm.reset()
    mm.update(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))
    want, skipped = _confusion_want(pred, gt, Cn)
    assert skipped == 1507
    assert np.array_equal(mm.confusion().cpu().numpy().reshape(-1), want) and int(mm.skipped()) == skipped
    out = mm.compute()
    tp = np.diag(want.reshape(Cn, Cn)).astype(np.float64)
    den = want.reshape(Cn, Cn).sum(0) + want.reshape(Cn, Cn).sum(1) - tp
    np.testing.assert_allclose(out["iou"].cpu().numpy(), tp / den, rtol=1e-12)


def test_no_host_synchronisation(mods, dev, crafted_iou):
    gtf, mg, M, MD = mods
    gts, preds = crafted_pair(SEEDS[0], dev)
    pm = MD.PoseMetricsDevice(C, full_thresholds(), {CKEY: CTHR}, keep_raw=16, device=dev)      # thresholds are uploaded here, once
    mm = MD.MaskMetricsDevice(C, device=dev)
    g = torch.Generator().manual_seed(0)
    pred_mask, gt_mask = (torch.randint(0, C, (2, 30, 40), generator=g).to(dev) for _ in range(2))
    gtf._rotation_table(dev)                                # built once per device on the host and uploaded
    before = dict(MD.counters)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.zeros(1, device=dev).item()
            enforced = False
        except RuntimeError:
            enforced = True
        if not enforced:
            pytest.skip("this torch build does not enforce set_sync_debug_mode('error')")
        dm = mg.batchwise_find_matches_device(preds, gts)
        pm.update(dm)
        pm.update(dm)
        table = pm.table()
        mm.update(pred_mask, gt_mask)
        scores = mm.compute()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert MD.counters["device"] == before["device"] + 2 and MD.counters["fallback"] == before["fallback"]
    assert int(pm.state[0]) == 2 and int(pm.state[7]) == 10 and np.isfinite(float(table["degree_error"]))
    assert int(mm.confusion().sum()) == 2400 and np.isfinite(float(scores["mean_iou"]))


def test_bit_identical_state(mods, dev, crafted_iou):
    thr = full_thresholds()
    (a, _), = run_crafted(mods, dev, thr, keep_raw=64)
    (b, _), = run_crafted(mods, dev, thr, keep_raw=64)
    assert torch.equal(a.state, b.state)
    for x, y in zip(a._raw, b._raw):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_fallback_gives_the_host_numbers(mods, dev, crafted_iou):
    """A DeviceMatches without `order` (more than 1024 instances a side: nothing ran on the device)."""
    gtf, mg, M, MD = mods
    thr = full_thresholds()
    pm = MD.PoseMetricsDevice(C, thr, {CKEY: CTHR}, keep_raw=64, device=dev)
    host = HostRoute(gtf, M)
    before = dict(MD.counters)
    for seed in SEEDS:
        gts, preds = crafted_pair(seed, dev)
        dm = mg.DeviceMatches(preds, gts)
        pm.update(dm)
        host.update(mg.batchwise_find_matches(preds, gts))
    assert MD.counters["fallback"] == before["fallback"] + 3 and MD.counters["device"] == before["device"]
    assert_same_table(pm, host, n_updates=3)
    aps, caps = pm.aps()
    assert_same_aps(aps, host.aps(thr, dev))
    assert_same_aps(caps, host.complex_aps(dev))
    (native, _), = run_crafted(mods, dev, thr, keep_raw=64)
    counts = [i for i in range(pm.state.numel()) if i not in (10, 11, 12)]
    assert torch.equal(pm.state[counts], native.state[counts])           # and the same counts as the kernel
    assert sorted(pm.raw()["3d_iou"]) == [1, 2, 5]
