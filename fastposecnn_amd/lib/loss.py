"""Drop-in for the loss classes `train.py` selects (F/lib/loss.py; criterion table F/train.py:159-187).

Pixel-wise mask losses take (pred, gt) = (forward()'s dict, the batch); matched losses take the dict of
`matching.batchwise_find_matches`: value [0] = ground truth, [1] = prediction.  Semantics follow the reference line by
line where it matters for the numbers: NaN (not zero) for "nothing matched", NaN-filtering before the mean, the symmetric
quaternion loss over 360 rotations about the object's axis in float64, XY / scales as a SUM of per-component means,
Z on log-depth.  `FocalLoss` restates pytorch_toolbelt.losses.FocalLoss (upstream, not in the reference tree; parity
unpinned) as the reference uses it: applied per class to LOG-SOFTMAX outputs as if they were logits.
"""
import ctypes
import functools

import torch
from torch import nn
from torch.nn.modules.loss import _Loss

import gpu_tensor_funcs as gtf


def _nan(gt_pred_matches=None):
    try:
        return torch.tensor(float('nan'), device=gt_pred_matches['instance_masks'].device).float()
    except Exception:
        return torch.tensor(float('nan'), device='cuda' if torch.cuda.is_available() else 'cpu').float()


# ---- mask losses (F/lib/loss.py:26-98) ---------------------------------------------------------------------------
class _MaskLossFn(torch.autograd.Function):
    """One of CE / CCE / Focal (which = 0 / 1 / 2) from the shared forward sums; its own backward launch, so the three loss
    objects stay independent autograd nodes (csrc/train.hip: k_mask_losses)."""

    @staticmethod
    def forward(ctx, logits, x, target, sums, which, ignore_cce, alpha, gamma):
        # x: the contiguous NCHW copy the forward sums were taken from (== logits when those are contiguous): the kernel
        # indexes plain NCHW, so the backward reads x, never a strided / channels_last `logits`
        ctx.save_for_backward(x, target, sums)
        ctx.args = (int(which), int(ignore_cce), float(alpha), float(gamma))
        return (sums[2 * which] / sums[2 * which + 1]).float()

    @staticmethod
    def backward(ctx, g):
        from fastposecnn_amd import _native as nat
        x, t, sums = ctx.saved_tensors
        which, ignore_cce, alpha, gamma = ctx.args
        w3 = torch.zeros(3, dtype=torch.float32, device=x.device)
        w3[which] = (g.double() / sums[2 * which + 1]).float()
        grad = torch.empty_like(x, memory_format=torch.contiguous_format)
        with torch.cuda.device(x.device):
            nat.check(nat.lib().fpc_mask_losses(nat.ptr(x), nat.ptr(t), x.shape[0], x.shape[1], x[0, 0].numel(), -100, ignore_cce,
                                                alpha, gamma, None, nat.ptr(w3), nat.ptr(grad), nat.stream()), "fpc_mask_losses")
        return grad, None, None, None, None, None, None, None


def _fused_mask_loss(which, logits, target, ignore_cce=-1, alpha=0.5, gamma=2):
    """CE / CCE / Focal (which = 0 / 1 / 2) for GPU f32 logits; the forward pass (all three sums) runs once per
    (logits, target, parameters) and is shared by the three loss objects of the criterion table, which are called one after
    the other on the same tensors.  None when the torch-op forms must run."""
    import os
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() >= 3 and logits.shape[1] <= 32
            and bool(int(os.environ.get("FPC_FUSED_MASK_LOSSES", "1")))):
        return None
    from fastposecnn_amd import _native as nat
    key = (int(ignore_cce), float(alpha), float(gamma))
    cached = getattr(logits, "_fpc_mask_losses", None)
    if cached is not None and cached[0] is target and cached[1] == key and cached[2] == logits._version:
        x, t, sums = cached[3]
    else:
        x = logits.detach()
        x = x if x.is_contiguous() else x.contiguous()
        t = target.to(torch.int64).contiguous()
        # (a target outside [0, C) other than the ignore indices contributes nothing here, where torch's own losses raise:
        # checking would cost a host synchronisation per training step; F/tools/dataset.py only produces class ids)
        sums = torch.zeros(6, dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            nat.check(nat.lib().fpc_mask_losses(nat.ptr(x), nat.ptr(t), x.shape[0], x.shape[1], x[0, 0].numel(), -100, key[0], key[1],
                                                key[2], nat.ptr(sums), None, None, nat.stream()), "fpc_mask_losses")
        logits._fpc_mask_losses = (target, key, logits._version, (x, t, sums))
    return _MaskLossFn.apply(logits, x, t, sums, which, *key)


class CE(_Loss):

    def __init__(self, ignore_index=-1):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, pred, gt):
        fused = _fused_mask_loss(0, pred['logits']['mask'], gt['mask'])
        if fused is not None:
            return fused
        return nn.functional.cross_entropy(pred['logits']['mask'], gt['mask'])


class CCE(_Loss):

    def __init__(self, from_logits=True, ignore_index=-1):
        super().__init__()
        self.from_logits = from_logits
        self.ignore_index = ignore_index

    def forward(self, pred, gt):
        fused = _fused_mask_loss(1, pred['logits']['mask'], gt['mask'], ignore_cce=self.ignore_index)
        if fused is not None:
            return fused
        y = nn.functional.log_softmax(pred['logits']['mask'], dim=1)
        return nn.functional.nll_loss(y, gt['mask'], ignore_index=self.ignore_index)


def focal_loss_with_logits(output, target, gamma=2.0, alpha=0.25):
    """pytorch_toolbelt.losses.functional.focal_loss_with_logits, reduction='mean', not normalised, no reduced threshold."""
    target = target.type(output.type())
    logpt = nn.functional.binary_cross_entropy_with_logits(output, target, reduction='none')
    pt = torch.exp(-logpt)
    loss = (1.0 - pt).pow(gamma) * logpt
    if alpha is not None:
        loss = loss * (alpha * target + (1 - alpha) * (1 - target))
    return loss.mean()


class FocalLoss(_Loss):
    """pytorch_toolbelt.losses.FocalLoss (multi-class): one-vs-rest binary focal loss per class, summed."""

    def __init__(self, alpha=None, gamma=2, ignore_index=None):
        super().__init__()
        self.alpha, self.gamma, self.ignore_index = alpha, gamma, ignore_index

    def forward(self, label_input, label_target):
        loss = 0
        not_ignored = label_target != self.ignore_index if self.ignore_index is not None else None
        for cls in range(label_input.size(1)):
            cls_target = (label_target == cls).long()
            cls_input = label_input[:, cls, ...]
            if not_ignored is not None:
                cls_target = cls_target[not_ignored]
                cls_input = cls_input[not_ignored]
            loss = loss + focal_loss_with_logits(cls_input, cls_target, gamma=self.gamma, alpha=self.alpha)
        return loss


class Focal(_Loss):

    def __init__(self, key='mask', from_logits=True, alpha=0.5, gamma=2, ignore_index=-1):
        super().__init__()
        self.from_logits = from_logits
        self.ignore_index = ignore_index
        self.alpha = alpha
        self.gamma = gamma

    def forward(self, pred, gt):
        fused = _fused_mask_loss(2, pred['logits']['mask'], gt['mask'], ignore_cce=self.ignore_index, alpha=self.alpha, gamma=self.gamma)
        if fused is not None:
            return fused
        y = nn.functional.log_softmax(pred['logits']['mask'], dim=1)       # the reference feeds log-probabilities (:91-98)
        return FocalLoss(alpha=self.alpha, gamma=self.gamma, ignore_index=self.ignore_index)(y, gt['mask'])


# ---- pixel-wise regression loss (:103-149) -----------------------------------------------------------------------
class MaskedMSELoss(_Loss):

    def __init__(self, key):
        super().__init__()
        self.key = key

    def forward(self, pred, gt):
        cat_mask = pred['categorical']['mask']
        if torch.sum(torch.logical_and(cat_mask != 0, gt['mask'] != 0)) == 0:
            return torch.tensor(float('nan'), device=cat_mask.device).float()
        y_pred, y_gt = pred[self.key], gt[self.key]
        binary = cat_mask != 0
        if len(y_pred.shape) > len(binary.shape):
            binary = torch.unsqueeze(binary, dim=1)
        return nn.functional.mse_loss(y_pred * binary, y_gt)


# ---- matched losses (:240-541) -----------------------------------------------------------------------------------
def dec_empty_check(function):
    """NaN when there are no matches or the key is absent (:240-270)."""

    @functools.wraps(function)
    def wrapper(self, gt_pred_matches=None, **kwargs):
        if gt_pred_matches is not None and self.key in gt_pred_matches.keys():
            return function(self, gt_pred_matches, **kwargs)
        return _nan(gt_pred_matches)

    return wrapper


def _mean_without_nan(loss):
    return torch.mean(loss[torch.isnan(loss) == False])      # noqa: E712 (the reference's filter, :299)


def _component_loss(loss_type):
    try:
        return {'L1': nn.L1Loss, 'SmoothL1': nn.SmoothL1Loss, 'L2': nn.MSELoss}[loss_type]()
    except KeyError:
        raise NotImplementedError(f"{loss_type} is an invalid loss function!")


class QLoss(_Loss):

    def __init__(self, key=None, eps=0.1):
        super().__init__()
        self.eps = eps
        self.key = key if key else 'quaternion'

    @dec_empty_check
    def forward(self, gt_pred_matches):
        gt, pred = gt_pred_matches[self.key][0], gt_pred_matches[self.key][1]
        non_symmetric = torch.where(gt_pred_matches['symmetric_ids'] == 0)[0]
        symmetric = torch.where(gt_pred_matches['symmetric_ids'] != 0)[0]
        loss = torch.cat((self.get_loss(gt[non_symmetric], pred[non_symmetric]),
                          self.get_symmetric_loss(gt[symmetric], pred[symmetric])), dim=0)
        return _mean_without_nan(loss)

    def get_loss(self, gt, pred):
        return self.dot_product_to_loss((gt * pred).sum(dim=1))          # diag(gt @ pred.T), :305

    def get_symmetric_loss(self, gt, pred):
        if gt.shape[0] == 0:
            return torch.tensor([float('nan')], device=gt.device)
        rot_e_gt, e_pred = gtf.quat_symmetric_tf(gt, pred)               # [n,360,4] each
        dot_product = torch.einsum('bij,bij->bi', e_pred.double(), rot_e_gt.double())
        return torch.min(self.dot_product_to_loss(dot_product), dim=1).values

    def dot_product_to_loss(self, dot_product):
        error = 1 - torch.pow(dot_product, 2)
        return torch.log(error + self.eps) - torch.log(torch.tensor(self.eps, device=error.device))


class RLoss(_Loss):

    def __init__(self, key=None, eps=0.1):
        super().__init__()
        self.eps = eps
        self.key = key if key else 'R'

    @dec_empty_check
    def forward(self, gt_pred_matches):
        gt, pred = gt_pred_matches[self.key][0], gt_pred_matches[self.key][1]
        traced = torch.einsum('bii->b', torch.bmm(torch.transpose(gt, 1, 2), pred))
        return _mean_without_nan(torch.acos((traced - 1) / 2))


class TLoss(_Loss):

    def __init__(self, key=None, eps=0.1):
        super().__init__()
        self.eps = eps
        self.key = key if key else 'T'

    @dec_empty_check
    def forward(self, gt_pred_matches):
        gt, pred = gt_pred_matches[self.key][0], gt_pred_matches[self.key][1]
        return _mean_without_nan((gt - pred).norm(dim=1))


class _ComponentwiseLoss(_Loss):
    """Sum over the components of the mean loss of each (XYLoss :431-468, ScalesLoss :505-541)."""
    default_key = None

    def __init__(self, key=None, loss_type='L2', eps=0.1):
        super().__init__()
        self.eps = eps
        self.key = key if key else self.default_key
        self.loss_func = _component_loss(loss_type)

    @dec_empty_check
    def forward(self, gt_pred_matches):
        gt, pred = gt_pred_matches[self.key][0], gt_pred_matches[self.key][1]
        return torch.sum(torch.stack([self.loss_func(gt[:, i], pred[:, i]) for i in range(gt.shape[1])]))


class XYLoss(_ComponentwiseLoss):
    default_key = 'xy'


class ScalesLoss(_ComponentwiseLoss):
    default_key = 'scales'


class ZLoss(_Loss):

    def __init__(self, key=None, loss_type='L2', eps=0.1):
        super().__init__()
        self.eps = eps
        self.key = key if key else 'z'
        self.loss_func = _component_loss(loss_type)

    @dec_empty_check
    def forward(self, gt_pred_matches):
        return self.loss_func(torch.log(gt_pred_matches[self.key][0]), torch.log(gt_pred_matches[self.key][1]))


class _PoseLoss(_Loss):
    """Losses over the assembled poses (F/lib/loss.py:546-626): NaN without matches, NaN-filtered mean."""

    def __init__(self, eps=0.1):
        super().__init__()
        self.eps = eps

    def forward(self, gt_pred_matches):
        if gt_pred_matches is None or 'RT' not in gt_pred_matches.keys():
            return _nan(gt_pred_matches)
        return _mean_without_nan(self.pair_loss(gt_pred_matches))


class Iou3dLoss(_PoseLoss):

    def pair_loss(self, m):
        return 1 - gtf.get_3d_ious(m['RT'][0], m['RT'][1], m['scales'][0], m['scales'][1])


class OffsetLoss(_PoseLoss):

    def pair_loss(self, m):
        return gtf.from_RTs_get_T_offset_errors(m['RT'][0], m['RT'][1]) / 10


def head_training_criterion(xy_loss_type='L2', z_loss_type='L2', scales_loss_type='L2'):
    """The criterion table of F/train.py:159-187 (D = where the inputs come from, weight = the factor in the task sum)."""
    return {
        'mask': {
            'loss_ce': {'D': 'pixel-wise', 'F': CE(), 'weight': 5.0},
            'loss_cce': {'D': 'pixel-wise', 'F': CCE(), 'weight': 5.0},
            'loss_focal': {'D': 'pixel-wise', 'F': Focal(), 'weight': 5.0},
        },
        'quaternion': {'loss_quat': {'D': 'matched', 'F': QLoss(key='quaternion'), 'weight': 0.1}},
        'xy': {'loss_xy': {'D': 'matched', 'F': XYLoss(key='xy', loss_type=xy_loss_type), 'weight': 0.01}},
        'z': {'loss_z': {'D': 'matched', 'F': ZLoss(key='z', loss_type=z_loss_type), 'weight': 0.1}},
        'scales': {'loss_scales': {'D': 'matched', 'F': ScalesLoss(key='scales', loss_type=scales_loss_type), 'weight': 0.1}},
    }


def total_loss(criterion, outputs, batch, gt_pred_matches, perform_matching=True):
    """PoseRegressionTask.shared_step's loss arithmetic (F/lib/pose_regressor.py:188-217, 265-307): per task the weighted
    sum of its non-NaN losses (NaN when all are NaN); the total is the sum of the non-NaN task sums.
    Returns (total, {task: {loss_name: value, 'task_total_loss': value}})."""
    dev = outputs['logits']['mask'].device
    total = torch.tensor(0.0, device=dev)
    report = {}
    for task_name, entries in criterion.items():
        losses = {}
        for loss_name, attrs in entries.items():
            if attrs['D'] == 'pixel-wise':
                losses[loss_name] = attrs['F'](outputs, batch)
            elif attrs['D'] == 'matched' and perform_matching:
                losses[loss_name] = attrs['F'](gt_pred_matches)
        weighted = [v * entries[k]['weight'] for k, v in losses.items() if not bool(torch.isnan(v))]
        task_total = torch.sum(torch.stack(weighted)) if weighted else torch.tensor(float('nan'), device=dev)
        losses['task_total_loss'] = task_total
        report[task_name] = losses
        if not bool(torch.isnan(task_total)):
            total = total + task_total
    return total, report


# ---- the matched half on the device (csrc/match_loss.hip) --------------------------------------------------------
counters = {'device': 0, 'fallback': 0}         # total_loss_device calls with matches: native launches / materialize() + total_loss

_MATCHED = ((QLoss, 'quaternion'), (XYLoss, 'xy'), (ZLoss, 'z'), (ScalesLoss, 'scales'))      # fpc_matched_losses' order
_LOSS_CODES = {nn.MSELoss: 0, nn.L1Loss: 1, nn.SmoothL1Loss: 2}                                 # FPC_LOSS_*
_dev_weights = {}


def _weights_on(weights, dev):
    """The four weights as a device tensor, filled without a host-to-device copy (which would synchronise)."""
    key = (weights, str(dev))
    if key not in _dev_weights:
        _dev_weights[key] = torch.stack([torch.full((), v, dtype=torch.float64, device=dev) for v in weights])
    return _dev_weights[key]


class _MatchedLossesFn(torch.autograd.Function):
    """(losses f64 [4], task totals f64 [4], their NaN-skipping sum f64 [1]) of the four matched losses over a DeviceMatches:
    one launch forward, one backward."""

    @staticmethod
    def forward(ctx, q, xy, z, s, dm, gt, cfg):
        from fastposecnn_amd import _native as nat
        eps, types, weights = cfg
        dev = q.device
        n1, n2 = gt[0].shape[0], q.shape[0]
        rot = gtf._rotation_table(dev)
        losses, tasks, total = (torch.empty(n, dtype=torch.float64, device=dev) for n in (4, 4, 1))
        best_rot = torch.empty(n1, dtype=torch.int32, device=dev)
        pred = tuple(t.detach().contiguous() for t in (q, xy, z, s))
        head = [nat.ptr(dm.order), nat.ptr(dm.match_pred), nat.ptr(dm.count), n1, n2, *[nat.ptr(t) for t in gt], *[nat.ptr(t) for t in pred],
                nat.ptr(rot), rot.shape[0], eps, *types, (ctypes.c_double * 4)(*weights)]
        with torch.cuda.device(dev):
            nat.check(nat.lib().fpc_matched_losses(*head, nat.ptr(losses), nat.ptr(tasks), nat.ptr(total), nat.ptr(best_rot),
                                                   nat.stream()), "fpc_matched_losses")
        ctx.keep = (head, dm, gt, pred, rot)                        # the tensors `head` points into
        ctx.save_for_backward(losses, best_rot, _weights_on(weights, dev))
        return losses, tasks, total

    @staticmethod
    def backward(ctx, g_losses, g_tasks, g_total):
        from fastposecnn_amd import _native as nat
        head, pred = ctx.keep[0], ctx.keep[3]
        losses, best_rot, w = ctx.saved_tensors
        g = (g_losses + w * (g_tasks + g_total)).contiguous()         # task_total[k] = w[k] * losses[k]; the total sums them
        grads = tuple(torch.empty_like(t) for t in pred)
        with torch.cuda.device(g.device):
            nat.check(nat.lib().fpc_matched_losses_backward(*head, nat.ptr(losses), nat.ptr(best_rot), nat.ptr(g), *[nat.ptr(t) for t in grads],
                                                            nat.stream()), "fpc_matched_losses_backward")
        return (*grads, None, None, None)


def _matched_plan(criterion, dm):
    """What fpc_matched_losses needs from the criterion and the two dicts, or None where total_loss must run: the matched
    entries are one QLoss, XYLoss, ZLoss and ScalesLoss on their own keys, each alone in its task; the eight value tensors
    are f32 on the current GPU; no ground truth requires grad; the sizes are within the device matching's limit."""
    if dm.order is None:
        return None
    found = {}
    for task, entries in criterion.items():
        for name, attrs in entries.items():
            if attrs['D'] != 'matched':
                continue
            fn = attrs['F']
            slot = [k for k, (cls, key) in enumerate(_MATCHED) if type(fn) is cls and fn.key == key]
            if not slot or slot[0] in found or len(entries) != 1:
                return None
            found[slot[0]] = (task, name, fn, float(attrs['weight']))
    if len(found) != 4:
        return None
    types = []
    for k in (1, 2, 3):
        lf = found[k][2].loss_func
        if type(lf) not in _LOSS_CODES or lf.reduction != 'mean' or getattr(lf, 'beta', 1.0) != 1.0:
            return None
        types.append(_LOSS_CODES[type(lf)])
    gts, preds = dm.gts, dm.preds
    dev = dm.order.device
    n1, n2 = dm.order.shape[0], preds['class_ids'].shape[0]
    tensors = []
    for d, n in ((gts, n1), (preds, n2)):
        for (_, key), width in zip(_MATCHED, (4, 2, 1, 3)):
            t = d.get(key)
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == (n, width)):
                return None
            tensors.append(t)
    sym = gts.get('symmetric_ids')
    if not (torch.is_tensor(sym) and sym.device == dev and tuple(sym.shape) == (n1,) and not sym.is_floating_point()):
        return None
    if dev.index != torch.cuda.current_device() or any(t.requires_grad for t in tensors[:4]):
        return None
    gt = tuple(t.detach().contiguous() for t in tensors[:4]) + (sym.to(torch.int64).contiguous(),)
    cfg = (float(found[0][2].eps), tuple(types), tuple(found[k][3] for k in range(4)))
    return found, gt, tensors[4:], cfg


def total_loss_device(criterion, outputs, batch, device_matches):
    """`total_loss` on a `matching.DeviceMatches` without a host synchronisation: the pixel-wise entries as they are, the
    four matched losses through fpc_matched_losses, the NaN rules of `total_loss` as tensor ops.  Same (total, report);
    every value is a 0-dim device tensor.  A criterion or tensors the native entry does not cover (see _matched_plan) go
    through materialize() and `total_loss`; `counters` says which of the two ran.  None: `total_loss(..., None)`."""
    if device_matches is None:
        return total_loss(criterion, outputs, batch, None)
    plan = _matched_plan(criterion, device_matches)
    if plan is None:
        counters['fallback'] += 1
        return total_loss(criterion, outputs, batch, device_matches.materialize())
    counters['device'] += 1
    found, gt, pred, cfg = plan
    losses, tasks, matched_total = _MatchedLossesFn.apply(*pred, device_matches, gt, cfg)
    losses32, tasks32 = losses.float(), tasks.float()                    # the dtypes of the classes: QLoss f64, the others f32
    by_task = {found[k][0]: {found[k][1]: (losses if k == 0 else losses32)[k], 'task_total_loss': (tasks if k == 0 else tasks32)[k]}
               for k in range(4)}
    dev = outputs['logits']['mask'].device
    total = torch.zeros((), device=dev)
    report = {}
    for task_name, entries in criterion.items():
        if task_name in by_task:
            report[task_name] = by_task[task_name]
            continue
        losses_t = {k: a['F'](outputs, batch) for k, a in entries.items() if a['D'] == 'pixel-wise'}
        if losses_t:
            weighted = torch.stack([v * entries[k]['weight'] for k, v in losses_t.items()])
            is_nan = torch.isnan(weighted)
            task_total = torch.where(is_nan.all(), torch.full_like(weighted[0], float('nan')),
                                     torch.where(is_nan, torch.zeros_like(weighted), weighted).sum())
        else:
            task_total = torch.full((), float('nan'), device=dev)
        losses_t['task_total_loss'] = task_total
        report[task_name] = losses_t
        total = total + torch.where(torch.isnan(task_total), torch.zeros_like(task_total), task_total)
    return total + matched_total[0], report
