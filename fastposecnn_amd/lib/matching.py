"""Drop-in for the reference's `matching.batchwise_find_matches` (F/lib/matching.py:226-325), the step right
after the inference path in `evaluate.py:148` and in every training step (`pose_regressor.py:184`).

The reference loops over the ground-truth classes and, per class, gathers the class's masks (1.2 MB each at
640x480), expands them to [n1,n2,H,W] twice (logical_and / logical_or) and reduces.  Here ONE native call
(`gtf.batchwise_get_2d_iou` -> fpc_mask_iou) yields the IoU of every (ground truth, prediction) pair from
bitsets; IoU is pairwise, so a class's matrix is a sub-matrix of it.  The per-class arg-max / validity logic
runs on that small matrix on the host with torch's own `max` (first maximum, NaN propagates — the reference's
semantics), and the matched tensors are gathered once per key.  One host synchronisation per call (the
reference has several per class: torch.unique, torch.where, boolean indexing).
Same quirk as the reference: sample ids are NOT compared — a ground-truth instance can match a prediction of
another image of the batch that overlaps it in pixel coordinates.

`batchwise_find_matches_device` is the same matching with the assignment on the device as well (fpc_match_assign,
csrc/match_loss.hip): two launches, no synchronisation; the result stays on the device for `loss.total_loss_device`
and becomes the dict above through `DeviceMatches.materialize()` (one synchronisation).
"""
import torch

import gpu_tensor_funcs as gtf
from fastposecnn_amd import _native as nat

KEYS_TO_STACK = [                      # matching.py:29-35
    'instance_masks',                  # Class
    'quaternion', 'R',                 # Rotation
    'scales',                          # Size
    'xy', 'z', 'T',                    # Translation
    'RT',                              # Transformation
]


def batchwise_find_matches(preds, gts):
    if not preds or not gts:                                  # :229-230
        return None
    if preds['class_ids'].shape[0] == 0:                      # :233-234
        return None
    if gts['class_ids'].shape[0] == 0:                        # no class to loop over: every list stays empty (:316-317)
        return None
    dev = gts['instance_masks'].device
    iou = gtf.batchwise_get_2d_iou(gts['instance_masks'], preds['instance_masks']).cpu()     # the one host sync
    g_cls = gts['class_ids'].cpu()
    p_cls = preds['class_ids'].cpu()
    g_idx, p_idx = [], []
    for class_id in torch.unique(g_cls):                      # ascending, as :252
        gi = torch.where(g_cls == class_id)[0]
        pi = torch.where(p_cls == class_id)[0]
        if gi.shape[0] == 0 or pi.shape[0] == 0:              # :263-264
            continue
        max_v, max_pred = torch.max(iou[gi][:, pi], dim=1)    # :276
        valid = max_v > 0                                     # :280 (NaN > 0 is False)
        if not bool(valid.any()):                             # :283-284
            continue
        g_idx.append(gi[valid])
        p_idx.append(pi[max_pred[valid]])
    if not g_idx:                                             # :316-317
        return None
    g_sel = torch.cat(g_idx).to(dev)
    p_sel = torch.cat(p_idx).to(dev)
    out = {
        'sample_ids': gts['sample_ids'][g_sel],               # :297-299
        'symmetric_ids': gts['symmetric_ids'][g_sel],
        'class_ids': gts['class_ids'][g_sel],                 # = the loop's class id, repeated
    }
    for key in gts.keys():                                    # stack_and_store_data, :41-59
        if key in KEYS_TO_STACK:
            out[key] = torch.stack((gts[key][g_sel], preds[key][p_sel]))
    return out


MAX_INSTANCES = 1024                   # FPC_MATCH_MAX_INSTANCES (include/fpc.h): the limit of n1 and of n2 on the device


class DeviceMatches:
    """The matching of `batchwise_find_matches_device`.  order i32 [n1]: the matched ground-truth indices in the output
    order of `batchwise_find_matches`, then -1; match_pred i32 [n1]: the matched prediction or -1; count i32 [1]; all on
    the device.  order is None beyond MAX_INSTANCES: nothing ran on the device, and materialize() is the host function."""

    def __init__(self, preds, gts, order=None, match_pred=None, count=None):
        self.preds, self.gts = preds, gts
        self.order, self.match_pred, self.count = order, match_pred, count
        self._done, self._dict = False, None

    def materialize(self):
        """Exactly what `batchwise_find_matches(preds, gts)` returns; synchronises once (the first call)."""
        if not self._done:
            self._dict = batchwise_find_matches(self.preds, self.gts) if self.order is None else self._gather()
            self._done = True
        return self._dict

    def _gather(self):
        n = int(self.count.item())                            # the one host sync
        if n == 0:
            return None
        g_sel = self.order[:n].long()
        p_sel = self.match_pred.long()[g_sel]
        gts, preds = self.gts, self.preds
        out = {'sample_ids': gts['sample_ids'][g_sel], 'symmetric_ids': gts['symmetric_ids'][g_sel],
               'class_ids': gts['class_ids'][g_sel]}
        for key in gts.keys():
            if key in KEYS_TO_STACK:
                out[key] = torch.stack((gts[key][g_sel], preds[key][p_sel]))
        return out


def batchwise_find_matches_device(preds, gts):
    """`batchwise_find_matches` without the host: None only where the host knows it from shapes alone."""
    if not preds or not gts:
        return None
    n1, n2 = gts['class_ids'].shape[0], preds['class_ids'].shape[0]
    if n1 == 0 or n2 == 0:
        return None
    nat.require_gpu(gts['instance_masks'], preds['instance_masks'], gts['class_ids'], preds['class_ids'],
                    what="batchwise_find_matches_device")
    if n1 > MAX_INSTANCES or n2 > MAX_INSTANCES:
        return DeviceMatches(preds, gts)
    dev = gts['instance_masks'].device
    iou = gtf.batchwise_get_2d_iou(gts['instance_masks'], preds['instance_masks'])
    if iou.device != dev or iou.dtype != torch.float32 or tuple(iou.shape) != (n1, n2):
        raise RuntimeError("batchwise_find_matches_device: the IoU matrix is not f32 [n1,n2] on the masks' device")
    iou = iou.contiguous()
    g_cls = gts['class_ids'].to(device=dev, dtype=torch.int64).contiguous()
    p_cls = preds['class_ids'].to(device=dev, dtype=torch.int64).contiguous()
    out = torch.empty(2 * n1 + 1, dtype=torch.int32, device=dev)
    order, match_pred, count = out[:n1], out[n1:2 * n1], out[2 * n1:]
    with torch.cuda.device(dev):
        nat.check(nat.lib().fpc_match_assign(nat.ptr(iou), nat.ptr(g_cls), nat.ptr(p_cls), n1, n2, nat.ptr(match_pred), nat.ptr(order),
                                             nat.ptr(count), nat.stream()), "fpc_match_assign")
    return DeviceMatches(preds, gts, order, match_pred, count)
