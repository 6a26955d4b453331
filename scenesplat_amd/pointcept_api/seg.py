"""Supervised semantic segmentation: ``DefaultSegmentorV2``, its two criteria and the ``SemSegEvaluator`` hook.

Registry names, constructor kwargs and forward contracts follow the reference (pointcept/models/default.py:37-74;
pointcept/models/losses/misc.py:35-62, losses/lovasz.py:121-256; engines/hooks/evaluator.py:106-240; utils/misc.py:167-179).
CrossEntropyLoss and the multiclass Lovasz-softmax run as ONE pass of csrc/seg_loss.hip each way: the reference's Python loop
over labels.unique() (a device->host sync) with one torch.sort per present class becomes one segmented radix sort over all
classes with the present-class flags kept on the device, so a training step of the segmentor can be captured and replayed.
The two criteria are separate objects (Criteria builds them from the config); like the language head (SF.lang_head_sums) they
find the segmentor's kernel pass by identity of (pred, target), so inside DefaultSegmentorV2 one kernel pass serves both.
"""
import weakref

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from .. import native as nv
from .. import pointops
from .engine import HookBase, get_world_size, is_main_process
from .lang import build_criteria
from .pdnorm import condition_key
from .registry import HOOKS, LOSSES, MODELS, build_model
from .structure import Point

_NO_IGNORE = -(1 << 63)          # ignore_index=None: a label value no row can carry


class _SegLossPair(torch.autograd.Function):
    """logits (n, C), labels (n) -> sums (4) = [ce_sum, n_valid, lovasz_sum, n_present]; gradients flow through sums[0], sums[2]."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, seen, lovasz):
        sums, rowstat, glov, present = nv.seg_loss_fwd(logits, labels, ignore_index, seen, lovasz)
        ctx.save_for_backward(logits, labels, rowstat, glov, present)
        ctx.ignore_index = ignore_index
        return sums

    @staticmethod
    def backward(ctx, dsums):
        logits, labels, rowstat, glov, present = ctx.saved_tensors
        coef = torch.stack([dsums[0], dsums[2]]).float().contiguous()
        return nv.seg_loss_bwd(logits, labels, ctx.ignore_index, rowstat, glov, present, coef), None, None, None, None


_PAIR_CACHE = {}


def seg_loss_sums(logits, labels, ignore_index, seen=None, seen_key=None, lovasz=True, share=False):
    """The kernel's sums for (logits, labels): the shared ones when DefaultSegmentorV2 made this pass for its criteria (same
    ignore_index and, for the Lovasz part, the same class_seen), else one new pass.  share=True (the segmentor) keeps the pass for
    the criteria that follow until seg_loss_release(); a loss called on its own never leaves one behind (a later call on the same
    tensors must not reuse sums whose graph a backward has freed)."""
    ent = _PAIR_CACHE.get("last")
    if ent is not None and ent["logits"]() is logits and ent["labels"]() is labels and ent["versions"] == (logits._version, labels._version) \
            and ent["ignore_index"] == ignore_index and (not lovasz or (ent["lovasz"] and ent["seen_key"] == seen_key)):
        return ent["sums"]
    sums = _SegLossPair.apply(logits, labels, ignore_index, seen, lovasz)
    if share:
        _PAIR_CACHE["last"] = dict(logits=weakref.ref(logits), labels=weakref.ref(labels), versions=(logits._version, labels._version),
                                   ignore_index=ignore_index, lovasz=lovasz, seen_key=seen_key, sums=sums)
    return sums


def seg_loss_release():
    _PAIR_CACHE.pop("last", None)


def _require_gpu(pred, name):
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda):
        raise RuntimeError(f"{name}: scenesplat_amd losses need GPU tensors (no CPU fallback)")


def _kernel_operands(pred, target, ignore_index, name):
    """(logits, int64 labels) in the kernel's contract, with the label range asserted on the device (no host sync)."""
    C = pred.shape[1]
    logits = pred if pred.dtype in (torch.float32, torch.bfloat16) else pred.float()
    # the caller's own tensors where they already fit: the two criteria find the shared pass by identity
    labels = target if target.dtype == torch.int64 and target.dim() == 1 and target.is_contiguous() else target.reshape(-1).long().contiguous()
    torch._assert_async(((labels == ignore_index) | ((labels >= 0) & (labels < C))).all(),
                        f"{name}: labels must lie in [0, num_classes) or equal ignore_index")
    return logits.contiguous(), labels


@LOSSES.register_module()
class CrossEntropyLoss(nn.Module):
    """losses/misc.py:35-62.  weight=None, label_smoothing=0 and reduction mean / sum run on the kernel; other settings call
    F.cross_entropy on the device (the weight is kept on the host until the first call instead of the reference's .cuda())."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction="mean", label_smoothing=0.0, loss_weight=1.0,
                 ignore_index=-1):
        super().__init__()
        if size_average is not None or reduce is not None:
            reduction = nn.modules.loss._Reduction.legacy_get_string(size_average, reduce)
        self.weight = torch.tensor(weight, dtype=torch.float32) if weight is not None else None
        self.reduction, self.label_smoothing, self.loss_weight, self.ignore_index = reduction, label_smoothing, loss_weight, ignore_index

    def _on_kernel(self, pred):
        return (self.weight is None and self.label_smoothing == 0 and self.reduction in ("mean", "sum") and pred.dim() == 2
                and 1 <= pred.shape[1] <= nv.SEG_MAX_CLASSES)

    def forward(self, pred, target):
        _require_gpu(pred, "CrossEntropyLoss")
        if not self._on_kernel(pred):
            w = self.weight.to(pred.device) if self.weight is not None else None
            loss = F.cross_entropy(pred.float(), target.long(), weight=w, ignore_index=self.ignore_index, reduction=self.reduction,
                                   label_smoothing=self.label_smoothing)
            return loss * self.loss_weight
        logits, labels = _kernel_operands(pred, target, self.ignore_index, "CrossEntropyLoss")
        sums = seg_loss_sums(logits, labels, int(self.ignore_index), lovasz=False)
        loss = sums[0] / sums[1] if self.reduction == "mean" else sums[0]     # no valid row: 0 / 0 = NaN, as torch
        return loss * self.loss_weight


@LOSSES.register_module()
class LovaszLoss(nn.Module):
    """losses/lovasz.py:213-256, mode="multiclass" with per_image=False (the Lovasz-softmax over all rows, averaged over the present
    classes).  A chunk without any valid row gives 0 with a zero gradient (the reference returns an empty tensor there)."""

    def __init__(self, mode, class_seen=None, per_image=False, ignore_index=None, loss_weight=1.0):
        super().__init__()
        if mode not in ("binary", "multiclass", "multilabel"):
            raise ValueError(f"LovaszLoss: unknown mode {mode!r}")
        if mode != "multiclass":
            raise NotImplementedError(f"LovaszLoss: mode={mode!r} (the Lovasz hinge) is not implemented; only mode='multiclass' runs "
                                      "on the HIP kernel")
        if per_image:
            raise NotImplementedError("LovaszLoss: per_image=True is not implemented; the HIP kernel averages over the whole chunk")
        self.mode, self.per_image, self.loss_weight = mode, per_image, loss_weight
        self.ignore_index = ignore_index
        self.class_seen = None if class_seen is None else sorted({int(c) for c in np.asarray(class_seen).reshape(-1).tolist()})
        self._seen_dev = {}

    def _ignore(self):
        return _NO_IGNORE if self.ignore_index is None else int(self.ignore_index)

    def _seen(self, C, device):
        """(C) uint8 mask on the device, built once per (C, device) -- before any capture, by the eager warm-up step."""
        if self.class_seen is None:
            return None, None
        key = (C, str(device))
        if key not in self._seen_dev:
            m = torch.zeros(C, dtype=torch.uint8)
            m[[c for c in self.class_seen if 0 <= c < C]] = 1
            self._seen_dev[key] = m.to(device)
        return self._seen_dev[key], tuple(self.class_seen)

    def sums(self, pred, target, share=False):
        _require_gpu(pred, "LovaszLoss")
        if pred.dim() != 2:
            raise NotImplementedError("LovaszLoss: logits must be (n, num_classes)")
        C = pred.shape[1]
        if C < 2:
            raise ValueError("LovaszLoss: multiclass mode needs num_classes >= 2")
        if C > nv.SEG_MAX_CLASSES:
            raise NotImplementedError(f"LovaszLoss: at most {nv.SEG_MAX_CLASSES} classes on the HIP kernel")
        logits, labels = _kernel_operands(pred, target, self._ignore(), "LovaszLoss")
        seen, seen_key = self._seen(C, pred.device)
        return seg_loss_sums(logits, labels, self._ignore(), seen, seen_key, lovasz=True, share=share)

    def forward(self, y_pred, y_true):
        s = self.sums(y_pred, y_true)
        return s[2] / s[3].clamp(min=1.0) * self.loss_weight


@MODELS.register_module()
class DefaultSegmentorV2(nn.Module):
    """models/default.py:37-74: backbone -> Linear seg_head -> criteria (train: dict(loss); eval: + seg_logits)."""

    def __init__(self, num_classes, backbone_out_channels, backbone=None, criteria=None):
        super().__init__()
        self.seg_head = nn.Linear(backbone_out_channels, num_classes) if num_classes > 0 else nn.Identity()
        self.backbone = build_model(backbone)
        self.criteria = build_criteria(criteria)

    def steady_key(self, host):
        """No host-side decision depends on the step's host values (the steady-state replay keys on this, not on epoch_progress)."""
        return condition_key(self.backbone, host)        # (a backbone with PDNorm layers: the selected norms are baked into a capture)

    def forward(self, input_dict):
        point = self.backbone(Point(input_dict))
        feat = point["feat"] if isinstance(point, dict) else point
        w = getattr(self.seg_head, "weight", None)
        if w is not None and not torch.is_autocast_enabled() and feat.dtype != w.dtype:
            feat = feat.to(w.dtype)              # a bf16 residual stream outside autocast (the evaluator's no_grad pass)
        seg_logits = self.seg_head(feat)
        if self.training:
            return dict(loss=self._criteria(seg_logits, input_dict["segment"]))
        if "segment" in input_dict.keys():
            return dict(loss=self._criteria(seg_logits, input_dict["segment"]), seg_logits=seg_logits)
        return dict(seg_logits=seg_logits)

    def _criteria(self, seg_logits, segment):
        """The criteria, with the loss pair's kernel pass made once up front when a LovaszLoss is among them (the cross-entropy
        object then reads its sums from the same pass)."""
        try:
            for c in self.criteria.criteria:
                if isinstance(c, LovaszLoss) and seg_logits.is_cuda and seg_logits.dim() == 2 \
                        and 2 <= seg_logits.shape[1] <= nv.SEG_MAX_CLASSES:
                    c.sums(seg_logits, segment, share=True)
                    break
            return self.criteria(seg_logits, segment)
        finally:
            seg_loss_release()


@HOOKS.register_module()
class SemSegEvaluator(HookBase):
    """engines/hooks/evaluator.py:106-240: after every epoch, the model in eval mode over trainer.val_loader; per-class
    intersection / union / target counts from the HIP kernel (csrc/seg_loss.hip), mIoU / mAcc / allAcc with the reference's
    formulas, comm_info["current_metric_value"] = mIoU for CheckpointSaver.  With origin_coord the predictions are carried to the
    original points by 1-NN (pointops.knn_query); enable_voting takes the majority over the vote_k nearest reported points on the
    GPU (pointops.neighbor_voting) instead of a CPU cKDTree.  The engine has no storage / writer: per-batch values and the
    per-epoch results stay in this hook (batch_history, results)."""

    def __init__(self, enable_voting=False, vote_k=25):
        self.enable_voting, self.vote_k = enable_voting, vote_k
        self.batch_history, self.results = [], []

    def _log(self, msg):
        tr = self.trainer
        if is_main_process() and getattr(tr, "logger", None):
            tr.logger(msg)

    def _meta(self):
        tr = self.trainer
        data = tr.cfg.get("data") or {}
        model = getattr(tr.model, "module", tr.model)
        num_classes = data.get("num_classes", getattr(getattr(model, "seg_head", None), "out_features", None))
        if num_classes is None:
            raise RuntimeError("SemSegEvaluator: cfg['data']['num_classes'] is not set and the model has no Linear seg_head")
        return int(num_classes), int(data.get("ignore_index", -1)), data.get("names")

    def after_epoch(self):
        if self.trainer.cfg.get("evaluate", True) and getattr(self.trainer, "val_loader", None) is not None:
            self.eval()

    def eval(self):
        tr = self.trainer
        C, ignore, names = self._meta()
        self._log(">>>>>>>>>>>>>>>> Start SemSegEvaluator >>>>>>>>>>>>>>>>")
        tr.model.eval()
        total = None
        losses, batches = [], []
        nbatch = len(tr.val_loader)
        for i, input_dict in enumerate(tr.val_loader):
            inp = {k: (v.to(tr.device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in input_dict.items()}
            with torch.no_grad():
                out = tr.model(inp)
                logits = out["seg_logits"]
                segment = inp["segment"]
                pred = None
                coords = inp["coord"] if "coord" in inp else None
                if "origin_coord" in inp:
                    idx, _ = pointops.knn_query(1, inp["coord"].float().contiguous(), inp["offset"].int().contiguous(),
                                                inp["origin_coord"].float().contiguous(), inp["origin_offset"].int().contiguous())
                    pred = logits.argmax(1)[idx.flatten().long()]
                    segment, coords = inp["origin_segment"], inp["origin_coord"]
                if self.enable_voting:
                    if pred is None:
                        pred = logits.argmax(1)
                    pred = pointops.neighbor_voting(coords, pred.int(), torch.ones(len(pred), dtype=torch.bool, device=pred.device),
                                                    self.vote_k, -1, C)
                seg64 = segment.reshape(-1).long().contiguous()
                if pred is None:
                    counts = nv.seg_iou(seg64, C, ignore, logits=logits.contiguous())
                else:
                    counts = nv.seg_iou(seg64, C, ignore, pred=pred.int().contiguous())
            if get_world_size() > 1:
                dist.all_reduce(counts)
            total = counts if total is None else total + counts
            loss = out.get("loss")
            losses.append(loss.detach().float() if loss is not None else None)
            batches.append(counts)
            if getattr(tr, "logger", None) is not None:
                info = "Test: [{}/{}] Loss {:.4f}".format(i + 1, nbatch, float(loss) if loss is not None else float("nan"))
                self._log(("Interp. " if "origin_coord" in inp else "") + info)
        if total is None:
            return
        inter, union, target = (total.cpu().numpy().astype(np.float64))
        iou_class = inter / (union + 1e-10)
        acc_class = inter / (target + 1e-10)
        m_iou, m_acc = float(np.mean(iou_class)), float(np.mean(acc_class))
        all_acc = float(sum(inter) / (sum(target) + 1e-10))
        lv = [float(v) for v in losses if v is not None]
        loss_avg = float(np.mean(lv)) if lv else float("nan")
        self.batch_history.append([dict(loss=(float(l) if l is not None else None), counts=c.cpu().numpy())
                                   for l, c in zip(losses, batches)])
        self.results.append(dict(epoch=tr.epoch + 1, loss=loss_avg, mIoU=m_iou, mAcc=m_acc, allAcc=all_acc, iou_class=iou_class,
                                 acc_class=acc_class, counts=total.cpu().numpy()))
        self._log("Val result: mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}.".format(m_iou, m_acc, all_acc))
        for c in range(C):
            self._log("Class_{idx}-{name} Result: iou/accuracy {iou:.4f}/{acc:.4f}".format(
                idx=c, name=names[c] if names is not None and c < len(names) else c, iou=iou_class[c], acc=acc_class[c]))
        self._log("<<<<<<<<<<<<<<<<< End Evaluation <<<<<<<<<<<<<<<<<")
        tr.comm_info["current_metric_value"] = m_iou
        tr.comm_info["current_metric_name"] = "mIoU"

    def after_train(self):
        self._log("Best {}: {:.4f}".format("mIoU", self.trainer.best_metric_value))
