"""lib/metrics_device.py without a GPU: what the accumulators derive from their integer state.  The state is built here
with numpy, word by word from the layout include/fpc.h documents, so these tests also pin that layout."""
import numpy as np
import pytest
import torch

from conftest import load_golden

THR = {"degree_error": [5., 10., 30., 60.], "3d_iou": [1., 10., 25., 50.], "offset_error": [5., 10., 50., 200.]}     # test_eval_losses.py's
CTHR = [[5, 10, 60], [5, 50, 200]]
KEYS = ("degree_error", "3d_iou", "offset_error")
C = 7


@pytest.fixture(scope="module")
def MD():
    import fastposecnn_amd.lib  # noqa: F401
    import metrics_device
    return metrics_device


def _state_from_raw(G):
    """The state the kernel would hold after seeing the golden's raw errors (IoU on the golden's percent scale)."""
    nthr, K = 12, 3
    s = np.zeros(16 + C * (6 + nthr + K), np.int64)
    for c in np.unique(G["cls"]):
        c = int(c)
        raw = [G[f"raw_{k}_{c}"].astype(np.float64) for k in KEYS]
        with np.errstate(invalid="ignore"):
            for m, k in enumerate(KEYS):
                s[16 + 6 * c + 2 * m] = np.sum(~np.isnan(raw[m]))
                s[16 + 6 * c + 2 * m + 1] = np.sum(np.isnan(raw[m]))
                for j, t in enumerate(np.asarray(THR[k], np.float32).astype(np.float64)):
                    s[16 + 6 * C + c * nthr + 4 * m + j] = np.sum(raw[m] > t if m == 1 else raw[m] < t)
            for k in range(K):
                s[16 + (6 + nthr) * C + c * K + k] = np.sum((raw[0] < CTHR[0][k]) & (raw[2] < CTHR[1][k]))
    return s


def test_aps_from_a_state_array(MD):
    G = load_golden("eval_losses.npz")
    pm = MD.PoseMetricsDevice(C, THR, {"degree_error+offset_error": CTHR}, device="cpu")
    s = _state_from_raw(G)
    assert pm.layout.words == s.size
    pm.load_state(s)
    aps, caps = pm.aps()
    classes = set(int(c) for c in np.unique(G["cls"])) | {"mean"}
    assert set(aps) == set(KEYS)
    for k in KEYS:
        assert set(aps[k]) == classes
        for c, v in aps[k].items():
            np.testing.assert_allclose(v.numpy(), G[f"aps_{k}_{c}"], rtol=1e-6, err_msg=f"{k} {c}")
    assert set(caps) == {"degree_error+offset_error"} and set(caps["degree_error+offset_error"]) == classes
    for c, v in caps["degree_error+offset_error"].items():
        np.testing.assert_allclose(v.numpy(), G[f"caps_{c}"], rtol=1e-6, err_msg=f"complex {c}")
    # the golden's NaN (class 1, degree) left the denominator: 2 valid of 3 pairs
    assert s[16 + 6 * 1] == 2 and s[16 + 6 * 1 + 1] == 1


def test_aps_leaves_out_a_class_without_valid_samples(MD):
    pm = MD.PoseMetricsDevice(4, {"degree_error": [5., 10.]}, device="cpu")
    s = np.zeros(pm.layout.words, np.int64)
    s[16 + 6 * 1], s[16 + 6 * 4 + 1 * 2: 16 + 6 * 4 + 1 * 2 + 2] = 4, (1, 3)      # class 1: 4 valid, hits 1 and 3
    s[16 + 6 * 2 + 1] = 2                                                          # class 2: NaN samples only
    pm.load_state(s)
    aps, caps = pm.aps()
    assert caps == {} and set(aps) == {"degree_error"} and set(aps["degree_error"]) == {1, "mean"}
    assert aps["degree_error"][1].tolist() == [0.25, 0.75] and aps["degree_error"]["mean"].tolist() == [0.25, 0.75]


def test_table_from_a_state_array(MD):
    pm = MD.PoseMetricsDevice(3, {}, device="cpu")
    s = np.zeros(pm.layout.words, np.int64)
    s[4:10] = (1, 4, 3, 4, 0, 5)                    # correct, total x 3: f32 percentages as the host classes take them
    s[10:13] = np.asarray([2.5, 40.0, 7.25]).view(np.int64)
    pm.load_state(s)
    t = pm.table()
    import metrics as M
    assert set(t) == set(M.head_training_metrics()["pose"])
    assert {k: float(v) for k, v in t.items()} == {"degree_error": 2.5, "degree_error_AP_5": 25.0, "iou_3d_mAP_0.25": 75.0,
                                                   "iou_3d_accuracy": 40.0, "offset_error_AP_5cm": 0.0, "offset_error": 7.25}


def test_mask_metrics_on_a_hand_written_confusion_matrix(MD):
    mm = MD.MaskMetricsDevice(3, device="cpu")
    #            pred 0  1  2
    conf = [[5, 1, 0],      # gt 0: TP 5, FN 1; FP (column 0 without the diagonal) 2
            [2, 4, 0],      # gt 1: TP 4, FN 2; FP 1
            [0, 0, 0]]      # class 2 is in neither plane
    mm.state[:9] = torch.tensor(conf).reshape(-1)
    assert mm.confusion().tolist() == conf
    out = mm.compute()
    iou, dice = [5 / 8, 4 / 7], [10 / 13, 8 / 11]
    for key, want in (("iou", iou), ("dice", dice), ("f1", dice)):
        got = out[key].tolist()
        assert got[:2] == pytest.approx(want, rel=1e-12) and np.isnan(got[2]), key
        assert float(out["mean_" + key]) == pytest.approx((want[0] + want[1]) / 2, rel=1e-12)       # the absent class is not a zero
        assert float(out["mean_" + key + "_no_bg"]) == pytest.approx(want[1], rel=1e-12)
    empty = MD.MaskMetricsDevice(3, device="cpu").compute()
    assert np.isnan(float(empty["mean_iou"])) and np.isnan(float(empty["mean_dice_no_bg"]))
    given = mm.compute(confusion=np.asarray(conf))
    assert given["iou"].tolist()[:2] == out["iou"].tolist()[:2]


def test_merge_adds_the_integer_state(MD):
    r = np.random.default_rng(3)
    a = MD.PoseMetricsDevice(4, {"degree_error": [5., 10.], "offset_error": [5.]}, [[5], [5]], device="cpu")
    b = MD.PoseMetricsDevice(4, {"degree_error": [5., 10.], "offset_error": [5.]}, [[5], [5]], device="cpu")
    sa, sb = (r.integers(0, 1000, a.layout.words).astype(np.int64) for _ in range(2))
    sa[10:13] = np.asarray([1.5, 2.5, 3.5]).view(np.int64)
    sb[10:13] = np.asarray([9.0, 9.0, 9.0]).view(np.int64)
    a.load_state(sa)
    b.load_state(sb)
    assert a.merge_(b) is a
    got = a.state.numpy()
    local = [2, 3, 10, 11, 12]                         # raw-log cursor / overflow and the running means: not defined across ranks
    counts = np.setdiff1d(np.arange(sa.size), local)
    assert np.array_equal(got[counts], (sa + sb)[counts]) and np.array_equal(got[local], sa[local])
    assert np.array_equal(b.state.numpy(), sb)
    with pytest.raises(ValueError):
        a.merge_(MD.PoseMetricsDevice(5, {"degree_error": [5., 10.], "offset_error": [5.]}, [[5], [5]], device="cpu"))
    m, n = MD.MaskMetricsDevice(3, device="cpu"), MD.MaskMetricsDevice(3, device="cpu")
    m.state += 2
    n.state += torch.arange(10)
    assert m.merge_(n).state.tolist() == [2 + i for i in range(10)]


def test_update_refuses_cpu_tensors_and_none_is_a_noop(MD):
    import matching as mg
    pm = MD.PoseMetricsDevice(3, {"degree_error": [5.]}, device="cpu")
    pm.update(None)
    assert not pm.state.any()
    z = torch.zeros
    d = {"class_ids": z(1, dtype=torch.int64), "symmetric_ids": z(1, dtype=torch.int64), "quaternion": z(1, 4), "RT": z(1, 4, 4),
         "scales": z(1, 3), "T": z(1, 3)}
    dm = mg.DeviceMatches(d, d, z(1, dtype=torch.int32), z(1, dtype=torch.int32), z(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pm.update(dm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MD.MaskMetricsDevice(3, device="cpu").update(z(2, 2, dtype=torch.int64), z(2, 2, dtype=torch.int64))
