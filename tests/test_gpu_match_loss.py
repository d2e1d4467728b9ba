"""The matching and the four matched losses on the device (csrc/match_loss.hip, matching.batchwise_find_matches_device,
loss.total_loss_device) against the host path they stand in for (matching.batchwise_find_matches, loss.total_loss) and
the reference's goldens.  Bars: those of test_eval_losses.py (losses rtol 2e-5 / atol 1e-6, gradients rtol 2e-3 /
atol 2e-5 max|g|); selections (order, match_pred, the materialised dict) are exact."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

GT_CLS = [2, 1, 1, 3, 1, 5, 1]
PRED_CLS = [1, 1, 2, 1, 4, 3, 2, 5]
NAN = float("nan")
IOU = [[.9, .9, .3, .9, .9, .9, .3, .9],            # tie inside class 2 -> p2; larger values of other classes ignored
       [.5, .5, .9, .2, .9, .9, .9, .9],            # tie p0 / p1 -> p0
       [.6, .1, .9, .0, .9, .9, .9, .9],            # p0 again (one prediction, two ground truths)
       [.9, .9, .9, .9, .9, .0, .9, .9],            # its class's only prediction has IoU 0 -> unmatched
       [.7, NAN, .9, .8, .9, .9, .9, .9],           # NaN inside its class -> unmatched
       [NAN, NAN, NAN, NAN, NAN, NAN, NAN, .25],    # NaN only in other classes -> p7
       [.0, .0, .9, .4, .9, .9, .9, .9]]            # p3
KEYS = ("quaternion", "xy", "z", "scales")
TASK = {"quaternion": "loss_quat", "xy": "loss_xy", "z": "loss_z", "scales": "loss_scales"}


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
    import loss as L
    import matching as mg
    return gtf, L, mg


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scene(cls, seed, dev, sym=None):
    """An AggData-like dict of len(cls) instances: unit quaternions, positive z; quaternion rows are replaced where a test
    needs to recognise them."""
    r = np.random.default_rng(seed)
    n = len(cls)
    q = r.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    d = {"class_ids": np.asarray(cls, np.int64), "sample_ids": r.integers(0, 3, n).astype(np.int64),
         "symmetric_ids": (r.integers(0, 3, n) if sym is None else np.full(n, sym)).astype(np.int64),
         "instance_masks": np.zeros((n, 4, 6), np.float32), "quaternion": q.astype(np.float32),
         "scales": (0.5 + r.random((n, 3))).astype(np.float32), "xy": (3 * r.normal(size=(n, 2))).astype(np.float32),
         "z": (500 + 1000 * r.random((n, 1))).astype(np.float32), "R": r.normal(size=(n, 3, 3)).astype(np.float32),
         "T": r.normal(size=(n, 3)).astype(np.float32), "RT": r.normal(size=(n, 4, 4)).astype(np.float32)}
    return {k: T(v, dev) for k, v in d.items()}


def _mask_part(dev):
    g = torch.Generator().manual_seed(0)
    return torch.randn(1, 7, 6, 8, generator=g).to(dev), {"mask": torch.randint(0, 7, (1, 6, 8), generator=g).to(dev)}


def _run(L, mg, crit, preds, gts, device, entry):
    """(values of the five figures, gradients on the prediction leaves and the mask logits) after backward through
    `entry` ('total' or one of KEYS); a fresh graph per call.  device: the new path, else the host path."""
    leaves = {k: preds[k].detach().clone().requires_grad_(True) for k in KEYS}
    p = dict(preds, **leaves)
    ml, batch = _mask_part(preds["quaternion"].device)
    ml.requires_grad_(True)
    out = {"logits": {"mask": ml}}
    if device:
        dm = mg.batchwise_find_matches_device(p, gts)
        total, rep = L.total_loss_device(crit, out, batch, dm)
    else:
        total, rep = L.total_loss(crit, out, batch, mg.batchwise_find_matches(p, gts))
    for v in [total] + [x for d in rep.values() for x in d.values()]:
        assert v.dim() == 0 and v.is_cuda
    target = total if entry == "total" else rep[entry][TASK[entry]]
    if target.requires_grad:
        target.backward()
    vals = {"total": total.detach()}
    for k in KEYS:
        vals[k] = rep[k][TASK[k]].detach()
        vals[k + "_task"] = rep[k]["task_total_loss"].detach()
    grads = {k: (torch.zeros_like(t) if t.grad is None else t.grad) for k, t in leaves.items()}
    grads["mask"] = torch.zeros_like(ml) if ml.grad is None else ml.grad
    return {k: v.cpu().numpy() for k, v in vals.items()}, {k: v.cpu().numpy() for k, v in grads.items()}


def _close_vals(got, want, keys=None):
    for k in keys or want:
        np.testing.assert_allclose(got[k], want[k], rtol=2e-5, atol=1e-6, equal_nan=True, err_msg=k)


def _close_grads(got, want, keys=None):
    for k in keys or want:
        np.testing.assert_allclose(got[k], want[k], rtol=2e-3, atol=2e-5 * max(1e-6, np.abs(want[k]).max()), err_msg=k)


def _compare(L, mg, crit, preds, gts):
    """Device path against host path: the five figures, and every gradient after backward through each figure alone."""
    for entry in ("total",) + KEYS:
        dv, dg = _run(L, mg, crit, preds, gts, True, entry)
        hv, hg = _run(L, mg, crit, preds, gts, False, entry)
        _close_vals(dv, hv)
        _close_grads(dg, hg)
    return dv, dg


@pytest.fixture
def crafted(mods, dev, monkeypatch):
    gtf, L, mg = mods
    iou = torch.tensor(IOU, dtype=torch.float32, device=dev)
    monkeypatch.setattr(gtf, "batchwise_get_2d_iou", lambda a, b: iou)
    gts, preds = _scene(GT_CLS, 1, dev), _scene(PRED_CLS, 2, dev)
    return gts, preds


def _patch_iou(monkeypatch, gtf, iou):
    monkeypatch.setattr(gtf, "batchwise_get_2d_iou", lambda a, b: iou)


def test_assignment_crafted(mods, dev, crafted):
    gtf, L, mg = mods
    gts, preds = crafted
    for d in (gts, preds):                              # row i of the quaternions is filled with i: identifies the rows
        n = d["quaternion"].shape[0]
        d["quaternion"] = torch.arange(n, dtype=torch.float32, device=dev).view(n, 1).expand(n, 4).contiguous()
    dm = mg.batchwise_find_matches_device(preds, gts)
    assert dm.order.dtype == dm.match_pred.dtype == dm.count.dtype == torch.int32
    assert dm.count.tolist() == [5]
    assert dm.order.tolist() == [1, 2, 6, 0, 5, -1, -1]
    assert dm.match_pred.tolist() == [2, 0, 0, -1, -1, 7, 3]
    want = mg.batchwise_find_matches(preds, gts)
    got = dm.materialize()
    assert got is dm.materialize()
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert got["quaternion"][0, :, 0].tolist() == [1, 2, 6, 0, 5] and got["quaternion"][1, :, 0].tolist() == [0, 0, 3, 2, 7]


def _dicts(g, tag):
    return {k[len(tag) + 1:]: g[k] for k in list(g.keys()) if k.startswith(tag + "_")}


def test_assignment_golden_and_oracle(mods, dev, oracle):
    """tests/golden/matching.npz through the real masks, as test_gpu_parity.py's matching test runs the host function."""
    gtf, L, mg = mods
    g = load_golden("matching.npz")
    td = lambda d: {k: T(v, dev) for k, v in d.items()}
    gts, preds, g2, p2 = (_dicts(g, t) for t in ("gts", "preds", "gts2", "preds2"))
    for (p, t, tag) in ((preds, gts, "out"), (p2, g2, "out2")):
        want = _dicts(g, tag)
        got = mg.batchwise_find_matches_device(td(p), td(t)).materialize()
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == torch.from_numpy(want[k]).dtype, k
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k
        orc = oracle.find_matches(p, t)
        assert sorted(got) == sorted(orc)
        for k in orc:
            assert np.array_equal(got[k].cpu().numpy(), orc[k]), k
    assert mg.batchwise_find_matches_device({k: v[:0] for k, v in td(preds).items()}, td(gts)) is None
    assert mg.batchwise_find_matches_device(None, td(gts)) is None and mg.batchwise_find_matches_device(td(preds), {}) is None
    assert mg.batchwise_find_matches_device(td(preds), {k: v[:0] for k, v in td(gts).items()}) is None
    none_on_device = mg.batchwise_find_matches_device({k: v[5:6] for k, v in td(preds).items()}, td(gts))   # nothing valid: only the
    assert none_on_device.count.tolist() == [0] and none_on_device.materialize() is None                   # device knows


def test_losses_golden(mods, dev, monkeypatch):
    """tests/golden/eval_losses.npz: ground truth i pairs with prediction i (same classes, identity IoU)."""
    gtf, L, mg = mods
    G = load_golden("eval_losses.npz")
    n = G["q0"].shape[0]
    _patch_iou(monkeypatch, gtf, torch.eye(n, device=dev))
    base = {"class_ids": T(G["cls"], dev), "instance_masks": torch.zeros((n, 4, 6), device=dev)}
    gts = dict(base, symmetric_ids=T(G["sym"], dev), **{k: T(G[a], dev) for k, a in zip(KEYS, ("q0", "xy0", "z0", "s0"))})
    preds = dict(base, **{k: T(G[a], dev) for k, a in zip(KEYS, ("q1", "xy1", "z1", "s1"))})
    crit = L.head_training_criterion()
    for key, name in zip(KEYS, ("QLoss", "XYLoss", "ZLoss", "ScalesLoss")):
        leaves = {k: preds[k].clone().requires_grad_(True) for k in KEYS}
        ml, batch = _mask_part(dev)
        dm = mg.batchwise_find_matches_device(dict(preds, **leaves), gts)
        assert dm.count.tolist() == [n]
        total, rep = L.total_loss_device(crit, {"logits": {"mask": ml}}, batch, dm)
        val, want = rep[key][TASK[key]], G[f"loss_{name}"]
        assert str(val.dtype).endswith(str(want.dtype)), (name, val.dtype, want.dtype)
        np.testing.assert_allclose(val.detach().cpu().numpy(), want, rtol=2e-5, atol=1e-6, err_msg=name)
        val.backward()
        gw = G[f"grad_{name}"]
        np.testing.assert_allclose(leaves[key].grad.cpu().numpy(), gw, rtol=2e-3, atol=2e-5 * max(1e-6, np.abs(gw).max()), err_msg=name)


def test_losses_doubly_matched_and_unmatched(mods, dev, crafted):
    """(a): prediction 0 is matched by two ground truths; predictions 1, 4, 5, 6 by none."""
    gtf, L, mg = mods
    gts, preds = crafted
    crit = L.head_training_criterion()
    _compare(L, mg, crit, preds, gts)
    dv, dg = _run(L, mg, crit, preds, gts, True, "total")
    for k in KEYS:
        assert np.isfinite(dv[k])
        assert not dg[k][[1, 4, 5, 6]].any() and dg[k][[0, 2, 3, 7]].any(), k


@pytest.mark.parametrize("sym", [0, 1])
def test_losses_all_plain_or_all_symmetric(mods, dev, crafted, sym):
    """(b), (c)"""
    gtf, L, mg = mods
    gts, preds = crafted
    gts["symmetric_ids"] = torch.full_like(gts["symmetric_ids"], sym)
    _compare(L, mg, L.head_training_criterion(), preds, gts)


def test_losses_nan_quaternion_is_dropped(mods, dev, crafted):
    """(d): prediction 3's quaternion is NaN: QLoss is the mean over the other pairs, and the gradients stay finite (the host
    path's quaternion gradient is NaN there: 0 x NaN)."""
    gtf, L, mg = mods
    gts, preds = crafted
    preds["quaternion"][3] = NAN
    crit = L.head_training_criterion()
    for entry in ("total",) + KEYS:
        dv, dg = _run(L, mg, crit, preds, gts, True, entry)
        hv, hg = _run(L, mg, crit, preds, gts, False, entry)
        _close_vals(dv, hv)
        assert np.isfinite(dv["quaternion"])
        assert all(np.isfinite(v).all() for v in dg.values())
        assert not dg["quaternion"][3].any()
        _close_grads(dg, hg, keys=("xy", "z", "scales", "mask"))


def test_losses_nan_z_leaves_the_total(mods, dev, crafted):
    """(e): prediction 2's z = -1: log gives NaN, loss_z and its task total are NaN and leave the total."""
    gtf, L, mg = mods
    gts, preds = crafted
    preds["z"][2] = -1.0
    crit = L.head_training_criterion()
    for entry in ("total", "quaternion", "xy", "scales"):
        dv, dg = _run(L, mg, crit, preds, gts, True, entry)
        hv, hg = _run(L, mg, crit, preds, gts, False, entry)
        _close_vals(dv, hv)
        _close_grads(dg, hg, keys=("quaternion", "xy", "scales", "mask"))
        assert np.isnan(dv["z"]) and np.isnan(dv["z_task"]) and np.isfinite(dv["total"])
        assert not dg["z"].any()
    dv, dg = _run(L, mg, crit, preds, gts, True, "z")      # backward through the NaN loss itself: exactly zero, not NaN
    assert not dg["z"].any()


@pytest.mark.parametrize("loss_type", ["L1", "SmoothL1", "L2"])
def test_losses_component_loss_types(mods, dev, crafted, loss_type):
    """(f).  xy differences straddle SmoothL1's |d| = 1."""
    gtf, L, mg = mods
    gts, preds = crafted
    _compare(L, mg, L.head_training_criterion(loss_type, loss_type, loss_type), preds, gts)


def test_losses_nothing_matched(mods, dev, crafted, monkeypatch):
    """(g)"""
    gtf, L, mg = mods
    gts, preds = crafted
    _patch_iou(monkeypatch, gtf, torch.zeros((7, 8), device=dev))
    crit = L.head_training_criterion()
    dv, dg = _run(L, mg, crit, preds, gts, True, "total")
    hv, hg = _run(L, mg, crit, preds, gts, False, "total")
    _close_vals(dv, hv)
    _close_grads(dg, hg)
    ml, batch = _mask_part(dev)
    mask_only, _ = L.total_loss(crit, {"logits": {"mask": ml}}, batch, None)
    np.testing.assert_allclose(dv["total"], mask_only.cpu().numpy(), rtol=2e-5, atol=1e-6)
    for k in KEYS:
        assert np.isnan(dv[k]) and np.isnan(dv[k + "_task"])
        assert not dg[k].any()
    leaves = {k: preds[k].clone().requires_grad_(True) for k in KEYS}
    dm = mg.batchwise_find_matches_device(dict(preds, **leaves), gts)
    assert dm.count.tolist() == [0] and dm.order.tolist() == [-1] * 7 and dm.match_pred.tolist() == [-1] * 7
    total, _ = L.total_loss_device(crit, {"logits": {"mask": ml}}, batch, dm)
    total.backward()
    for k in KEYS:                                          # the matched part is in the graph: zeros, written by the kernel
        assert leaves[k].grad is not None and not leaves[k].grad.any()


def test_no_host_synchronisation(mods, dev, crafted):
    gtf, L, mg = mods
    gts, preds = crafted
    crit = L.head_training_criterion()
    leaves = {k: preds[k].clone().requires_grad_(True) for k in KEYS}
    p = dict(preds, **leaves)
    ml, batch = _mask_part(dev)
    ml.requires_grad_(True)
    gtf._rotation_table(dev)                                # built once per device on the host and uploaded
    L._dev_weights.clear()                                  # the first call with a criterion's weights is under the mode too
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.zeros(1, device=dev).item()
            enforced = False
        except RuntimeError:
            enforced = True
        if not enforced:
            pytest.skip("this torch build does not enforce set_sync_debug_mode('error')")
        before = dict(L.counters)
        dm = mg.batchwise_find_matches_device(p, gts)
        total, rep = L.total_loss_device(crit, {"logits": {"mask": ml}}, batch, dm)
        total.backward()
        assert L.counters["device"] == before["device"] + 1 and L.counters["fallback"] == before["fallback"]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.isfinite(float(total)) and all(t.grad is not None for t in leaves.values()) and ml.grad is not None


def test_bit_identical_runs_and_counters(mods, dev, crafted):
    gtf, L, mg = mods
    gts, preds = crafted
    crit = L.head_training_criterion()
    before = dict(L.counters)
    av, ag = _run(L, mg, crit, preds, gts, True, "total")
    bv, bg = _run(L, mg, crit, preds, gts, True, "total")
    for k in av:
        assert av[k].tobytes() == bv[k].tobytes(), k
    for k in ag:
        assert ag[k].tobytes() == bg[k].tobytes(), k
    assert L.counters["device"] == before["device"] + 2 and L.counters["fallback"] == before["fallback"]


@pytest.mark.parametrize("case", ["extra_loss", "float64_gt"])
def test_fallback_gives_the_host_numbers(mods, dev, crafted, case):
    gtf, L, mg = mods
    gts, preds = crafted
    crit = L.head_training_criterion()
    if case == "extra_loss":
        crit["R"] = {"loss_R": {"D": "matched", "F": L.RLoss(key="R"), "weight": 0.1}}
    else:
        gts["quaternion"] = gts["quaternion"].double()
    before = dict(L.counters)
    ml, batch = _mask_part(dev)
    out = {"logits": {"mask": ml}}
    got, got_rep = L.total_loss_device(crit, out, batch, mg.batchwise_find_matches_device(preds, gts))
    want, want_rep = L.total_loss(crit, out, batch, mg.batchwise_find_matches(preds, gts))
    assert L.counters["fallback"] == before["fallback"] + 1 and L.counters["device"] == before["device"]
    assert torch.equal(got, want)
    for task in want_rep:
        assert list(got_rep[task]) == list(want_rep[task])
        for k, v in want_rep[task].items():
            assert torch.equal(got_rep[task][k], v) or bool(torch.isnan(v) & torch.isnan(got_rep[task][k])), (task, k)
