"""Evaluation metrics accumulated on the device: what `evaluate.py` and the validation step report, without moving a match
to the host ("Metrics on the device").

`PoseMetricsDevice` consumes the `DeviceMatches` of `matching.batchwise_find_matches_device` where it lies: ONE launch per
update (fpc_pose_metrics_update, csrc/pose_metrics.hip), no host synchronisation, no shape that depends on the number of
matches.  Its state holds integer counts per class and threshold, from which `aps()` gives the dicts of
`gtf.calculate_aps` / `gtf.calculate_complex_aps` over evaluate.py:238-292's per-class raw errors, and the six scalars of
`metrics.head_training_metrics()['pose']` (`table()`).  `lib/metrics.py` keeps its behaviour; nothing uses this module by default.

`MaskMetricsDevice` accumulates the confusion matrix of the arg-max mask against the ground-truth mask (fpc_confusion_update,
csrc/confusion.hip) and derives per-class IoU / dice / F1 from it by the textbook definitions.  These are NOT claimed equal
to `pl.metrics.functional` of Lightning 1.0, which the reference's table uses (F/train.py:190-207): that package is in
neither tree, so its conventions (reduction, absent classes, background) cannot be pinned.
"""
import numpy as np
import torch

import gpu_tensor_funcs as gtf
from fastposecnn_amd import _native as nat

POSE_KEYS = ('degree_error', '3d_iou', 'offset_error')         # metric 0, 1, 2 of the state
COMPLEX_KEY = 'degree_error+offset_error'
TABLE_NAMES = ('degree_error', 'degree_error_AP_5', 'iou_3d_mAP_0.25', 'iou_3d_accuracy', 'offset_error_AP_5cm', 'offset_error')
HEADER = 16                                                    # include/fpc.h: the state's fixed words
W_UPDATES, W_SKIPPED, W_CURSOR, W_OVERFLOW = 0, 1, 2, 3
W_CORRECT = (4, 6, 8)                                          # + 1: total
W_MEAN = (10, 11, 12)                                          # f64 bits: DegreeError, Iou3dAccuracy, OffsetError
_LOCAL_WORDS = (W_CURSOR, W_OVERFLOW) + W_MEAN                 # merge_ leaves these alone

counters = {'device': 0, 'fallback': 0}        # PoseMetricsDevice.update calls with matches: native launches / materialize() + host


class PoseStateLayout:
    """Word offsets of fpc_pose_metrics_update's state (include/fpc.h) for C classes and the given threshold counts."""

    def __init__(self, num_classes, n_deg, n_iou, n_off, n_complex):
        self.C, self.n, self.K = int(num_classes), (int(n_deg), int(n_iou), int(n_off)), int(n_complex)
        self.nthr = sum(self.n)
        self.words = HEADER + self.C * (6 + self.nthr + self.K)

    def samples(self, c, metric):
        """Word of class c's non-NaN samples of `metric`; the NaN samples are the next word."""
        return HEADER + 6 * c + 2 * metric

    def hits(self, c, metric):
        """(first word, count) of class c's per-threshold hits of `metric`."""
        return HEADER + 6 * self.C + c * self.nthr + sum(self.n[:metric]), self.n[metric]

    def complex_hits(self, c):
        return HEADER + (6 + self.nthr) * self.C + c * self.K, self.K


def _thr(values, device):
    """Thresholds as the host compare sees them: `operator(f64 data, f32 thresholds)` widens the f32 values."""
    return torch.as_tensor(values).detach().to(torch.float32).to(torch.float64).reshape(-1).contiguous().to(device)


def _default_device(device):
    if device is not None:
        return torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


class PoseMetricsDevice:
    """thresholds: {'degree_error': [..], '3d_iou': [..], 'offset_error': [..]} (any subset; `calculate_aps`'s
    metrics_threshold; degree and offset hit with <, IoU with >, IoU on its own 0..1 scale as evaluate.py has it).
    complex_thresholds: {'degree_error+offset_error': [2,K]} (or the [2,K] array), `calculate_complex_aps`'s.
    keep_raw: capacity in pairs of the optional raw log behind `raw()`.  table_thresholds: those of `table()`'s three APs.

    Rules: a NaN error is counted apart and leaves `aps()`'s denominators, as `calculate_aps` drops it;
    it stays in the totals of iou_3d_mAP / offset_error_AP and leaves degree_error_AP's, as the host classes have it.  An
    update without a match leaves the state untouched, running means included.  A class id outside 1..num_classes-1
    never indexes anything: the pair enters `table()` and the raw log only and is counted in `skipped()`."""

    def __init__(self, num_classes, thresholds, complex_thresholds=None, keep_raw=0, table_thresholds=(5, 0.25, 5), device=None):
        self.device = _default_device(device)
        self.num_classes = int(num_classes)
        unknown = set(thresholds) - set(POSE_KEYS)
        if unknown:
            raise ValueError(f"PoseMetricsDevice: unknown metrics {sorted(unknown)}")
        self._keys = [k for k in thresholds]                    # aps() answers for these, in this order
        self._thr = [_thr(thresholds.get(k, []), self.device) for k in POSE_KEYS]
        if isinstance(complex_thresholds, dict):
            if list(complex_thresholds) != [COMPLEX_KEY]:
                raise ValueError(f"PoseMetricsDevice: the one complex metric is '{COMPLEX_KEY}'")
            complex_thresholds = complex_thresholds[COMPLEX_KEY]
        self._has_complex = complex_thresholds is not None
        cx = torch.as_tensor(complex_thresholds if self._has_complex else [[], []])
        if cx.dim() != 2 or cx.shape[0] != 2:
            raise ValueError("PoseMetricsDevice: complex thresholds are [2,K]: degree row, offset row")
        self._thr_cx = _thr(cx, self.device)
        self._thr_table = _thr(list(table_thresholds), self.device)
        if self._thr_table.numel() != 3:
            raise ValueError("PoseMetricsDevice: table_thresholds are (degree, 3-D IoU, offset)")
        self.layout = PoseStateLayout(self.num_classes, *(t.numel() for t in self._thr), cx.shape[1])
        if self.device.type == 'cuda':
            words = nat.lib().fpc_pose_metrics_state_words(self.num_classes, *self.layout.n, self.layout.K)
            if words != self.layout.words:
                raise ValueError("PoseMetricsDevice: class or threshold counts beyond fpc_pose_metrics_update's limits")
        self.state = torch.zeros(self.layout.words, dtype=torch.int64, device=self.device)
        self.capacity = int(keep_raw)
        cap = max(self.capacity, 1)
        self._raw = (torch.zeros(cap, dtype=torch.float64, device=self.device), torch.zeros(cap, dtype=torch.float32, device=self.device),
                     torch.zeros(cap, dtype=torch.float32, device=self.device), torch.zeros(cap, dtype=torch.int32, device=self.device))

    # ---- accumulation -------------------------------------------------------------------------------------------------
    def update(self, device_matches):
        """None: nothing.  A DeviceMatches beyond matching.MAX_INSTANCES (order is None) goes through materialize() and
        the host functions (`counters['fallback']`); every other one is one launch and no synchronisation."""
        dm = device_matches
        if dm is None:
            return
        if dm.order is None:
            counters['fallback'] += 1
            self._update_host(dm.materialize())
            return
        gts, preds = dm.gts, dm.preds
        nat.require_gpu(self.state, dm.order, gts['quaternion'], preds['quaternion'], what="PoseMetricsDevice.update")
        n1, n2 = gts['class_ids'].shape[0], preds['class_ids'].shape[0]
        dev = self.state.device
        f = gtf._f32c
        g = [f(gts[k]) for k in ('quaternion', 'RT', 'scales', 'T')]
        p = [f(preds[k]) for k in ('quaternion', 'RT', 'scales', 'T')]
        for side, n in ((g, n1), (p, n2)):
            if any(t.device != dev or t.numel() != n * w for t, w in zip(side, (4, 16, 3, 3))):
                raise RuntimeError("PoseMetricsDevice.update: quaternion [n,4], RT [n,4,4], scales [n,3], T [n,3] on the state's device")
        sym = gts['symmetric_ids'].to(device=dev, dtype=torch.int64).contiguous()
        cls = gts['class_ids'].to(device=dev, dtype=torch.int64).contiguous()
        if sym.numel() != n1 or dm.order.numel() != n1 or dm.match_pred.numel() != n1:
            raise RuntimeError("PoseMetricsDevice.update: symmetric_ids, order and match_pred are [n1]")
        rot = gtf._rotation_table(dev)
        L = self.layout
        raw = self._raw if self.capacity else (None,) * 4
        with torch.cuda.device(dev):
            nat.check(nat.lib().fpc_pose_metrics_update(
                nat.ptr(dm.order), nat.ptr(dm.match_pred), nat.ptr(dm.count), n1, n2, nat.ptr(g[0]), nat.ptr(g[1]), nat.ptr(g[2]),
                nat.ptr(g[3]), nat.ptr(sym), nat.ptr(cls), nat.ptr(p[0]), nat.ptr(p[1]), nat.ptr(p[2]), nat.ptr(p[3]), nat.ptr(rot),
                rot.shape[0], nat.ptr(self._thr[0]), L.n[0], nat.ptr(self._thr[1]), L.n[1], nat.ptr(self._thr[2]), L.n[2],
                nat.ptr(self._thr_cx), L.K, nat.ptr(self._thr_table), self.num_classes, nat.ptr(self.state), nat.ptr(raw[0]),
                nat.ptr(raw[1]), nat.ptr(raw[2]), nat.ptr(raw[3]), self.capacity, nat.stream()), "fpc_pose_metrics_update")
        counters['device'] += 1

    def _update_host(self, m):
        """The kernel's fold with the host functions on a materialised match (synchronises)."""
        if m is None or 'quaternion' not in m:
            return
        q, RT, sc, T = m['quaternion'], m['RT'], m['scales'], m['T']
        n = q.shape[1]
        sym = m['symmetric_ids']
        deg = torch.empty(n, dtype=torch.float64, device=q.device)
        plain, symm = torch.where(sym == 0)[0], torch.where(sym != 0)[0]
        if plain.numel():
            deg[plain] = gtf.get_raw_quat_distance(q[0][plain], q[1][plain]).double()
        if symm.numel():
            deg[symm] = gtf.get_symmetric_quat_distance(q[0][symm], q[1][symm]).double()
        iou = gtf.get_3d_ious(RT[0], RT[1], sc[0], sc[1]).float()
        off = gtf.from_Ts_get_offset_error(T[0], T[1]).float()
        means = (torch.mean(deg[~torch.isnan(deg)]), torch.mean(iou * 100), gtf.from_RTs_get_T_offset_errors(RT[0], RT[1]))
        deg, iou, off, cls = deg.cpu().numpy(), iou.cpu().numpy(), off.cpu().numpy(), m['class_ids'].cpu().numpy()
        s = self.state.cpu().numpy().copy()
        L, thr = self.layout, [t.cpu().numpy() for t in self._thr]
        cx, tt = self._thr_cx.cpu().numpy().reshape(2, -1), self._thr_table.cpu().numpy()
        vals = (deg, iou.astype(np.float64), off.astype(np.float64))
        with np.errstate(invalid='ignore'):
            hit = lambda m_, v, t: (v > t) if m_ == 1 else (v < t)
            for i in range(n):
                c = int(cls[i])
                if not 1 <= c < L.C:
                    s[W_SKIPPED] += 1
                    continue
                for m_ in range(3):
                    s[L.samples(c, m_) + int(np.isnan(vals[m_][i]))] += 1
                    a, k = L.hits(c, m_)
                    s[a:a + k] += hit(m_, vals[m_][i], thr[m_])
                a, k = L.complex_hits(c)
                s[a:a + k] += (deg[i] < cx[0]) & (vals[2][i] < cx[1])
            for m_ in range(3):
                s[W_CORRECT[m_]] += int(np.sum(hit(m_, vals[m_], tt[m_])))
                s[W_CORRECT[m_] + 1] += int(np.sum(~np.isnan(deg))) if m_ == 0 else n
        f = s.view(np.float64)
        for w, v in zip(W_MEAN, means):
            f[w] = (f[w] + float(v)) / 2
        cur = int(s[W_CURSOR])
        k = max(0, min(self.capacity, cur + n) - min(self.capacity, cur))
        if k:
            for buf, v in zip(self._raw, (deg, iou, off, cls)):
                buf[cur:cur + k] = torch.from_numpy(np.ascontiguousarray(v[:k])).to(buf.dtype).to(buf.device)
        s[W_UPDATES] += 1
        s[W_CURSOR] = cur + n
        if self.capacity:
            s[W_OVERFLOW] += n - k
        self.state.copy_(torch.from_numpy(s))

    def reset(self):
        self.state.zero_()

    def load_state(self, words):
        """Replaces the state by `words` (i64 [layout.words]): a saved or externally reduced state."""
        w = torch.as_tensor(words, dtype=torch.int64).reshape(-1)
        if w.numel() != self.layout.words:
            raise ValueError("PoseMetricsDevice.load_state: not this layout")
        self.state.copy_(w)

    def merge_(self, other):
        """Adds another accumulator's integer state (the same classes and thresholds), e.g. another rank's.  NOT defined for
        the running means (the reference reduces those across ranks by 'mean') nor for the raw log: both stay this one's."""
        if (other.layout.C, other.layout.n, other.layout.K) != (self.layout.C, self.layout.n, self.layout.K):
            raise ValueError("PoseMetricsDevice.merge_: different classes or thresholds")
        add = other.state.to(self.state.device).clone()
        add[list(_LOCAL_WORDS)] = 0
        self.state += add
        return self

    # ---- results --------------------------------------------------------------------------------------------------------
    def table(self):
        """The six values of metrics.head_training_metrics()['pose'] under the same names; device tensors, no synchronisation."""
        s = self.state
        pct = lambda w: (s[w].float() / s[w + 1].float()) * 100
        mean = s[W_MEAN[0]:W_MEAN[2] + 1].view(torch.float64)
        return {'degree_error': mean[0], 'degree_error_AP_5': pct(W_CORRECT[0]), 'iou_3d_mAP_0.25': pct(W_CORRECT[1]),
                'iou_3d_accuracy': mean[1], 'offset_error_AP_5cm': pct(W_CORRECT[2]), 'offset_error': mean[2]}

    def skipped(self):
        return self.state[W_SKIPPED]

    def overflow(self):
        return self.state[W_OVERFLOW]

    def aps(self):
        """(calculate_aps's dict, calculate_complex_aps's dict) from the counts: per metric {class_id: tensor[len(thresholds)],
        'mean': ...}.  A class without a valid (non-NaN) sample of a metric is left out of that metric's dict and mean;
        the complex metric counts every pair of a class, as `torch.less` on a NaN counts a miss.  Synchronises (once)."""
        s = self.state.cpu()
        L, dev = self.layout, self.state.device
        simple = {}
        for key in self._keys:
            m_ = POSE_KEYS.index(key)
            per = {}
            for c in range(1, L.C):
                valid = int(s[L.samples(c, m_)])
                if valid:
                    a, k = L.hits(c, m_)
                    per[c] = (s[a:a + k] / valid).to(dev)
            per['mean'] = self._mean(per, L.n[m_], dev)
            simple[key] = per
        compl = {}
        if self._has_complex:
            per = {}
            for c in range(1, L.C):
                pairs = int(s[L.samples(c, 0)] + s[L.samples(c, 0) + 1])
                if pairs:
                    a, k = L.complex_hits(c)
                    per[c] = (s[a:a + k] / pairs).to(dev)
            per['mean'] = self._mean(per, L.K, dev)
            compl[COMPLEX_KEY] = per
        return simple, compl

    @staticmethod
    def _mean(per, n, dev):
        if not per:
            return torch.full((n,), float('nan'), device=dev)
        return torch.mean(torch.stack(list(per.values())).float(), dim=0)

    def raw(self):
        """The logged errors per class in evaluate.py's raw_data layout: {metric: {class_id: tensor}}, pairs in the order
        they were matched.  Unlike get_quat_distance's list the degree errors keep the pair order and their NaNs, so the
        three lists of a class stay aligned (calculate_aps drops the NaNs itself).  Synchronises."""
        n = min(int(self.state[W_CURSOR]), self.capacity)
        deg, iou, off, cls = (b[:n] for b in self._raw)
        out = {k: {} for k in POSE_KEYS}
        for c in torch.unique(cls).tolist():
            at = torch.where(cls == c)[0]
            out['degree_error'][int(c)], out['3d_iou'][int(c)], out['offset_error'][int(c)] = deg[at], iou[at], off[at]
        return out


class MaskMetricsDevice:
    """Confusion matrix of (ground-truth label, predicted label) over every pixel seen, rows = ground truth.  Pixels with a
    label outside [0, num_classes) in either plane (ignore labels, negative values) are left out and counted in `skipped()`.

    `compute()`: per class IoU = TP / (TP + FP + FN) and dice = F1 = 2 TP / (2 TP + FP + FN), NaN where the denominator is
    0 (the class is in neither plane), and their means over the classes present, with and without the background class 0.
    Textbook definitions on the accumulated matrix; NOT claimed equal to Lightning 1.0's pl.metrics.functional (see the
    module docstring)."""

    MAX_CLASSES = 32

    def __init__(self, num_classes, device=None):
        if not 1 <= int(num_classes) <= self.MAX_CLASSES:
            raise ValueError("MaskMetricsDevice: 1 <= num_classes <= 32")
        self.num_classes = int(num_classes)
        self.device = _default_device(device)
        self.state = torch.zeros(self.num_classes ** 2 + 1, dtype=torch.int64, device=self.device)

    def update(self, pred_mask, gt_mask):
        """pred_mask, gt_mask: integer label planes of the same shape (the engine's cat['mask'] and the batch's mask) on the
        GPU.  One launch, no synchronisation."""
        nat.require_gpu(self.state, pred_mask, gt_mask, what="MaskMetricsDevice.update")
        if pred_mask.shape != gt_mask.shape:
            raise RuntimeError("MaskMetricsDevice.update: the two planes differ in shape")
        dev = self.state.device
        pred = pred_mask.to(device=dev, dtype=torch.int64).contiguous()
        gt = gt_mask.to(device=dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            nat.check(nat.lib().fpc_confusion_update(nat.ptr(pred), nat.ptr(gt), pred.numel(), self.num_classes, nat.ptr(self.state),
                                                     nat.stream()), "fpc_confusion_update")

    def confusion(self):
        """i64 [C,C], [gt, pred]; a view of the state."""
        C = self.num_classes
        return self.state[:C * C].view(C, C)

    def skipped(self):
        return self.state[-1]

    def reset(self):
        self.state.zero_()

    def merge_(self, other):
        if other.num_classes != self.num_classes:
            raise ValueError("MaskMetricsDevice.merge_: different class counts")
        self.state += other.state.to(self.state.device)
        return self

    def compute(self, confusion=None):
        """From this accumulator's matrix, or from a given [C,C] one.  Tensors on the matrix's device, no synchronisation."""
        m = (self.confusion() if confusion is None else torch.as_tensor(confusion)).double()
        tp = torch.diagonal(m)
        fp, fn = m.sum(dim=0) - tp, m.sum(dim=1) - tp
        iou = tp / (tp + fp + fn)                                # 0 / 0 = NaN: the class is absent from both planes
        dice = 2 * tp / (2 * tp + fp + fn)
        out = {'iou': iou, 'dice': dice, 'f1': dice}
        for k, v in list(out.items()):
            out['mean_' + k] = _nanmean(v)
            out['mean_' + k + '_no_bg'] = _nanmean(v[1:])
        return out


def _nanmean(v):
    keep = ~torch.isnan(v)
    return torch.where(keep, v, torch.zeros_like(v)).sum() / keep.sum()      # no class present: 0 / 0 = NaN
