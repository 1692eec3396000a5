"""Focal and smooth-L1 losses.

Behavioural spec: keras-retinanet ``losses.focal(alpha=0.25, gamma=2.0)`` and
``losses.smooth_l1(sigma=3.0)`` compiled at ``/root/reference/train.py:99-102``
(SURVEY §2.8.6).  Both are normalised by max(1, #positive anchors in the *local* batch).

* ``focal_keras`` / ``smooth_l1_keras`` take the reference's dense ``y_true`` tensors
  (labels or regression targets with the anchor state as last column) and probabilities
  -- a literal fp32 re-statement used as the test oracle.
* ``focal_loss`` / ``smooth_l1_loss`` are the training path: logits in, compact targets
  (state int8, label int32, regression f32).  On the GPU they dispatch to one fused HIP
  kernel (``csrc/kernels/losses.hip``) that writes the loss partial sums *and* dlogits in
  a single pass over the 16M-logit/image classification tensor; the torch fallback is
  used on the CPU.
* ``iou_loss`` (GIoU / DIoU / CIoU of the decoded boxes, ``Trainer(regression_loss=...)``) takes smooth-L1's place
  on request: the torch expression here is the CPU path and the oracle of ``iou_loss_kernel``.
* ``quality_loss`` (Quality Focal / Varifocal loss, ``Trainer(classification_loss=...)``) takes focal's place on
  request: the label class of a positive anchor is trained towards ``quality_targets``, the IoU of its predicted box.
  The torch expression here is the CPU path and, in float64, the oracle of ``csrc/kernels/quality_loss.hip``.
* ``distribution_focal_loss`` (``RetinaNet(regression_bins=K)``) trains a distribution box head next to the box loss on
  its integral deltas (``ops.boxes.box_integral``); the kernel is ``csrc/kernels/box_dist.hip``.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional

import torch

KERAS_EPSILON = 1e-7
# Keras' binary_crossentropy clips probabilities to [eps, 1-eps] (fp32) and converts back
# to logits; in logit space that is a clamp to [LOGIT_LO, LOGIT_HI].  1-eps rounds to
# 0.99999988 in fp32, hence the asymmetric bounds.
_P_HI = float(torch.tensor(1.0 - KERAS_EPSILON, dtype=torch.float32))
LOGIT_LO = math.log(KERAS_EPSILON / (1.0 - KERAS_EPSILON))
LOGIT_HI = math.log(_P_HI / (1.0 - _P_HI))


def focal_keras(y_true: torch.Tensor, y_pred: torch.Tensor, alpha: float = 0.25, gamma: float = 2.0) -> torch.Tensor:
    """Reference focal loss.  y_true (B, A, C+1) labels + state column; y_pred (B, A, C) probs."""
    labels = y_true[..., :-1]
    state = y_true[..., -1]
    keep = state != -1
    labels = labels[keep]
    cls = y_pred[keep]
    alpha_f = torch.where(labels == 1, torch.full_like(labels, alpha), torch.full_like(labels, 1 - alpha))
    fw = torch.where(labels == 1, 1 - cls, cls)
    fw = alpha_f * fw ** gamma
    out = cls.clamp(KERAS_EPSILON, _P_HI)
    logit = torch.log(out / (1 - out))
    bce = torch.clamp(logit, min=0) - logit * labels + torch.log1p(torch.exp(-logit.abs()))
    normalizer = torch.clamp((state == 1).sum().to(y_pred.dtype), min=1.0)
    return (fw * bce).sum() / normalizer


def smooth_l1_keras(y_true: torch.Tensor, y_pred: torch.Tensor, sigma: float = 3.0) -> torch.Tensor:
    """Reference smooth-L1.  y_true (B, A, 5) targets + state column; y_pred (B, A, 4)."""
    s2 = sigma ** 2
    tgt = y_true[..., :4]
    state = y_true[..., 4]
    pos = state == 1
    d = (y_pred[pos] - tgt[pos]).abs()
    loss = torch.where(d < 1.0 / s2, 0.5 * s2 * d ** 2, d - 0.5 / s2)
    normalizer = torch.clamp(pos.sum().to(y_pred.dtype), min=1.0)
    return loss.sum() / normalizer


# ----------------------------------------------------------------------------------------
# training path (compact targets, logits)
# ----------------------------------------------------------------------------------------

def num_positives(state: torch.Tensor) -> torch.Tensor:
    return (state == 1).sum()


def _focal_torch(logits, state, label, alpha, gamma):
    x = logits.float()
    B, A, C = x.shape
    keep = (state != -1)
    pos = (state == 1)
    y = torch.zeros_like(x)
    y.scatter_(2, label.clamp(0, C - 1).long()[..., None], pos[..., None].to(x.dtype))
    p = torch.sigmoid(x)
    alpha_t = torch.where(y == 1, torch.full_like(x, alpha), torch.full_like(x, 1 - alpha))
    fw = alpha_t * torch.where(y == 1, 1 - p, p) ** gamma
    xc = x.clamp(LOGIT_LO, LOGIT_HI)
    bce = torch.where(y == 1, torch.nn.functional.softplus(-xc), torch.nn.functional.softplus(xc))
    loss = (fw * bce * keep[..., None].to(x.dtype)).sum()
    return loss / torch.clamp(pos.sum().to(x.dtype), min=1.0)


def _smooth_l1_torch(reg, reg_t, state, sigma):
    s2 = sigma ** 2
    pos = (state == 1)
    d = (reg.float() - reg_t.float()).abs()
    l = torch.where(d < 1.0 / s2, 0.5 * s2 * d * d, d - 0.5 / s2)
    l = (l * pos[..., None].to(l.dtype)).sum()
    return l / torch.clamp(pos.sum().to(l.dtype), min=1.0)


IOU_KINDS = ("giou", "diou", "ciou")
IOU_EPS = 1e-7


def iou_loss_rows(anchors: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, kind: str,
                  alpha: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-row GIoU / DIoU / CIoU loss of predicted against target deltas, (N, 4) each with their anchors
    (N, 4), in the dtype of the inputs.  Both boxes are ``bbox_transform_inv`` of their deltas; the predicted one
    has its corners ordered (a linear decode can flip).  ``alpha``: CIoU's trade-off weight per row instead of the
    one these boxes give (the backward holds it fixed; so does a check of the gradient against differences)."""
    from .boxes import bbox_transform_inv
    eps = IOU_EPS
    gx1, gy1, gx2, gy2 = bbox_transform_inv(anchors, target).unbind(-1)
    qx1, qy1, qx2, qy2 = bbox_transform_inv(anchors, pred).unbind(-1)
    px1, px2 = torch.minimum(qx1, qx2), torch.maximum(qx1, qx2)
    py1, py2 = torch.minimum(qy1, qy2), torch.maximum(qy1, qy2)
    iw = (torch.minimum(px2, gx2) - torch.maximum(px1, gx1)).clamp_min(0)
    ih = (torch.minimum(py2, gy2) - torch.maximum(py1, gy1)).clamp_min(0)
    inter = iw * ih
    union = (px2 - px1) * (py2 - py1) + (gx2 - gx1) * (gy2 - gy1) - inter + eps
    iou = inter / union
    cw = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    ch = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    if kind == "giou":
        c = cw * ch + eps
        return 1 - iou + (c - union) / c
    c2 = cw * cw + ch * ch + eps
    rho2 = ((px1 + px2 - gx1 - gx2) ** 2 + (py1 + py2 - gy1 - gy2) ** 2) / 4
    diou = 1 - iou + rho2 / c2
    if kind == "diou":
        return diou
    if kind != "ciou":
        raise ValueError("kind must be one of {}, got {!r}".format(IOU_KINDS, kind))
    v = 4 / math.pi ** 2 * (torch.atan((gx2 - gx1) / (gy2 - gy1 + eps)) - torch.atan((px2 - px1) / (py2 - py1 + eps))) ** 2
    if alpha is None:
        alpha = (v / (1 - iou + v + eps)).detach()    # a constant in the backward, as in the paper
    return diou + alpha * v


def _iou_loss_torch(reg, reg_t, state, anchors, kind, weight):
    A = anchors.shape[0]
    pos = (state == 1).reshape(-1, A)
    an = anchors.float()[None].expand(pos.shape[0], A, 4)[pos]
    l = iou_loss_rows(an, reg.float().reshape(-1, A, 4)[pos], reg_t.float().reshape(-1, A, 4)[pos], kind).sum()
    return weight * l / torch.clamp(pos.sum().to(l.dtype), min=1.0)


def iou_loss(reg: torch.Tensor, reg_t: torch.Tensor, state: torch.Tensor, anchors: torch.Tensor, kind: str,
             weight: float = 1.0, backend: str = "auto") -> torch.Tensor:
    """``weight`` x the GIoU / DIoU / CIoU loss of the decoded boxes over positive anchors; reg / reg_t (B, A, 4)
    deltas, anchors (A, 4)."""
    from . import native
    if kind not in IOU_KINDS:
        raise ValueError("kind must be one of {}, got {!r}".format(IOU_KINDS, kind))
    if backend == "auto":
        backend = "hip" if (reg.is_cuda and native.available()) else "torch"
    if backend == "hip":
        return native.IoULossFn.apply(reg, reg_t, state, anchors, kind, weight)
    return _iou_loss_torch(reg, reg_t, state, anchors, kind, weight)


CLS_KINDS = ("qfl", "vfl")
VFL_ALPHA = 0.75


def quality_targets(anchors: torch.Tensor, reg: torch.Tensor, reg_t: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """Per row the soft target of the IoU-aware classification losses: the IoU of the decoded predicted box with the
    decoded target box, exactly ``iou_loss_rows``' ``iou``; 0 where the state is not 1.  reg / reg_t (B, A, 4) deltas,
    anchors (A, 4), state (B, A); returns (B, A) in the dtype of ``reg``, detached (a constant in the backward)."""
    from .boxes import bbox_transform_inv
    A = anchors.shape[0]
    dt = reg.dtype
    an = anchors.to(dt)[None]
    with torch.no_grad():
        gx1, gy1, gx2, gy2 = bbox_transform_inv(an, reg_t.to(dt).reshape(-1, A, 4)).unbind(-1)
        qx1, qy1, qx2, qy2 = bbox_transform_inv(an, reg.reshape(-1, A, 4)).unbind(-1)
        px1, px2 = torch.minimum(qx1, qx2), torch.maximum(qx1, qx2)
        py1, py2 = torch.minimum(qy1, qy2), torch.maximum(qy1, qy2)
        iw = (torch.minimum(px2, gx2) - torch.maximum(px1, gx1)).clamp_min(0)
        ih = (torch.minimum(py2, gy2) - torch.maximum(py1, gy1)).clamp_min(0)
        inter = iw * ih
        union = (px2 - px1) * (py2 - py1) + (gx2 - gx1) * (gy2 - gy1) - inter + IOU_EPS
        q = inter / union
        return torch.where(state.reshape(-1, A) == 1, q, torch.zeros_like(q))


def _softplus(x):
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def _quality_torch(logits, reg, reg_t, state, label, anchors, kind, quality=None):
    x = logits if logits.dtype == torch.float64 else logits.float()
    B, A, C = x.shape
    if quality is None:
        q = quality_targets(anchors, reg.to(x.dtype), reg_t, state)
    else:
        q = torch.where(state == 1, quality.detach().to(x.dtype).reshape(B, A), torch.zeros((), dtype=x.dtype,
                                                                                             device=x.device))
    pos = (state == 1)
    keep = (state != -1)[..., None].to(x.dtype)
    t = torch.zeros_like(x)
    t.scatter_(2, label.clamp(0, C - 1).long()[..., None], q[..., None])
    sp = _softplus(x)
    # sigmoid as exp(-softplus(-x)): the backward of torch.sigmoid, p (1 - p), loses 1 - p from x = 17 on in fp32
    p = torch.exp(-_softplus(-x))
    if kind == "qfl":
        elem = (p - t) ** 2 * (sp - t * x)
    else:
        elem = torch.where(t > 0, t * (sp - t * x), VFL_ALPHA * p * p * sp)
    loss = (elem * keep).sum()
    return loss / torch.clamp(pos.sum().to(x.dtype), min=1.0)


def quality_loss(logits: torch.Tensor, reg: Optional[torch.Tensor], reg_t: Optional[torch.Tensor], state: torch.Tensor,
                 label: torch.Tensor, anchors: Optional[torch.Tensor], kind: str, backend: str = "auto",
                 quality: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Quality Focal Loss (``kind="qfl"``: Li et al. 2020, beta = 2) or Varifocal Loss (``"vfl"``: Zhang et al. 2021,
    alpha = 0.75, gamma = 2) on logits (B, A, C): the label class of a positive anchor is trained towards
    ``quality_targets`` (the IoU of its predicted box, no gradient into ``reg``), every other class towards 0.  Summed
    over the anchors whose state is not -1 and divided by max(1, #positives), without Keras' probability clip.  The
    torch expression computes in fp32, or in float64 when the logits are float64 (the kernel's oracle).  ``quality``
    (B, A): the soft target itself (a task-aligned assignment's, ``ops.anchors.tal_targets_bbox``) in place of the IoU;
    ``reg``, ``reg_t`` and ``anchors`` are then not read and may be None.  Only the torch expression takes it: no kernel
    reads a given target, and asking the HIP backend for one is an error."""
    from . import native
    if kind not in CLS_KINDS:
        raise ValueError("kind must be one of {}, got {!r}".format(CLS_KINDS, kind))
    if backend == "auto":
        backend = "hip" if (logits.is_cuda and native.available()) else "torch"
    if quality is not None and backend == "hip":
        raise RuntimeError("quality_loss: quality_loss.hip has no HIP kernel that reads a given target; "
                           "backend=\"torch\" is the expression")
    if backend == "hip":
        return native.QualityLossFn.apply(logits, reg, reg_t, state, label, anchors, kind)
    return _quality_torch(logits, reg, reg_t, state, label, anchors, kind, quality)


DFL_WEIGHT = 0.25
DFL_CLAMP_MARGIN = 0.01
_FALLBACK_WARNED = set()


def _dfl_torch(logits, reg_t, state, K, R, weight):
    dt = logits.dtype if logits.dtype == torch.float64 else torch.float32
    l = logits.to(dt).reshape(-1, 4, K)
    pos = (state == 1).reshape(-1)
    D = 2.0 * R / (K - 1)
    u = ((reg_t.to(dt).reshape(-1, 4) + R) / D).clamp(0, (K - 1) - DFL_CLAMP_MARGIN)
    il = u.floor()
    wr = u - il
    wl = 1 - wr
    il = il.long()
    logp = torch.log_softmax(l, dim=-1)              # no log of a rounded probability
    per = -(wl * logp.gather(-1, il[..., None])[..., 0] + wr * logp.gather(-1, il[..., None] + 1)[..., 0])
    s = (per * pos[:, None].to(dt)).sum()
    return weight * s / (4 * torch.clamp(pos.sum().to(dt), min=1.0))


def distribution_focal_loss(logits: torch.Tensor, reg_t: torch.Tensor, state: torch.Tensor, K: int, R: float = 8.0,
                            weight: float = DFL_WEIGHT, backend: str = "auto") -> torch.Tensor:
    """``weight`` x Distribution Focal Loss (Li et al. 2020, section 3.3) of a distribution box head: logits
    (B, A, 4 * K), per side K bins ``ops.boxes.box_bins(K, R)``; the target delta ``reg_t`` (B, A, 4) is clamped into the
    bins' range (0.01 of a bin below the last value) and the two bins that bracket it are trained towards it with the
    weights of a linear interpolation, on the log-softmax.  Summed over the sides of the rows with state 1 and divided
    by 4 max(1, #positives): no weighting by the quality score.  The torch expression computes in fp32, or in float64
    when the logits are float64 (the kernel's oracle)."""
    from . import native
    K = int(K)
    if K < 2 or logits.shape[-1] != 4 * K:
        raise ValueError("distribution_focal_loss: logits (..., 4 * K) with K >= 2 expected, got {} with K = {}".format(
            tuple(logits.shape), K))
    if backend == "auto":
        backend = "hip" if (logits.is_cuda and native.available()) else "torch"
    if backend == "hip":
        try:
            return native.DistributionFocalLossFn.apply(logits, reg_t, state, K, float(R), float(weight))
        except native.NotServed:
            key = ("dfl", K, logits.dtype)
            if key not in _FALLBACK_WARNED:
                _FALLBACK_WARNED.add(key)
                warnings.warn("box_dist.hip does not serve {} bins of {}: the distribution focal loss runs as the torch "
                              "expression".format(K, logits.dtype))
    return _dfl_torch(logits, reg_t, state, K, float(R), float(weight))


def focal_loss(logits: torch.Tensor, state: torch.Tensor, label: torch.Tensor,
               alpha: float = 0.25, gamma: float = 2.0, backend: str = "auto") -> torch.Tensor:
    """Focal loss on logits (B, A, C) with compact targets; returns a scalar fp32."""
    from . import native
    if backend == "auto":
        backend = "hip" if (logits.is_cuda and native.available()) else "torch"
    if backend == "hip":
        return native.FocalLossFn.apply(logits, state, label, alpha, gamma)
    return _focal_torch(logits, state, label, alpha, gamma)


def smooth_l1_loss(reg: torch.Tensor, reg_t: torch.Tensor, state: torch.Tensor,
                   sigma: float = 3.0, backend: str = "auto") -> torch.Tensor:
    """Smooth-L1 over positive anchors; reg/reg_t (B, A, 4)."""
    from . import native
    if backend == "auto":
        backend = "hip" if (reg.is_cuda and native.available()) else "torch"
    if backend == "hip":
        return native.SmoothL1Fn.apply(reg, reg_t, state, sigma)
    return _smooth_l1_torch(reg, reg_t, state, sigma)
