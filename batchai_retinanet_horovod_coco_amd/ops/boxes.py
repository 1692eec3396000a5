"""Box decode / clip / NMS / detection filtering (prediction graph).

Behavioural spec: keras-retinanet ``layers.RegressBoxes``, ``layers.ClipBoxes`` and
``layers.FilterDetections`` used by ``retinanet_bbox`` at ``/root/reference/train.py:95,408``
(SURVEY §2.8.8).  The torch code here is the oracle and the CPU path; on a GPU the fused HIP
kernels in ``csrc/kernels/detect.hip`` (decode+clip, bitmask NMS) are dispatched through
``ops.native``.
"""
from __future__ import annotations

import warnings
from typing import Optional, Tuple

import torch

from .anchors import BOX_MEAN, BOX_STD


def bbox_transform_inv(anchors: torch.Tensor, deltas: torch.Tensor, mean=BOX_MEAN, std=BOX_STD) -> torch.Tensor:
    """Inverse of the corner-offset encoding.  anchors (..., A, 4), deltas (..., A, 4)."""
    aw = anchors[..., 2] - anchors[..., 0]
    ah = anchors[..., 3] - anchors[..., 1]
    d = deltas * std + mean
    x1 = anchors[..., 0] + d[..., 0] * aw
    y1 = anchors[..., 1] + d[..., 1] * ah
    x2 = anchors[..., 2] + d[..., 2] * aw
    y2 = anchors[..., 3] + d[..., 3] * ah
    return torch.stack([x1, y1, x2, y2], dim=-1)


MAX_REGRESSION_BINS = 32
_FALLBACK_WARNED = set()


def check_regression_bins(bins, rng: float = 8.0):
    """``(bins, range)`` as the model keeps them: 0 bins (the plain 4-number head) or 2..32 with a range > 0."""
    bins = int(bins or 0)
    if bins != 0 and not 2 <= bins <= MAX_REGRESSION_BINS:
        raise ValueError("regression_bins must be 0 or 2..{}, got {}".format(MAX_REGRESSION_BINS, bins))
    if not float(rng) > 0:
        raise ValueError("regression_range must be > 0, got {}".format(rng))
    return bins, float(rng)


def box_bins(K: int, R: float, dtype=torch.float32, device=None) -> torch.Tensor:
    """The K bin values ``v_i = -R + i * D``, ``D = 2R / (K - 1)``, in the head's delta units."""
    return (-R + torch.arange(K, dtype=torch.float64, device=device) * (2.0 * R / (K - 1))).to(dtype)


def _box_integral_torch(logits: torch.Tensor, K: int, R: float) -> torch.Tensor:
    dt = logits.dtype if logits.dtype == torch.float64 else torch.float32
    l = logits.to(dt).reshape(logits.shape[:-1] + (4, K))
    p = torch.softmax(l, dim=-1)                     # subtracts the maximum
    return (p * box_bins(K, R, dt, logits.device)).sum(-1).to(logits.dtype)


def box_integral(logits: torch.Tensor, K: int, R: float = 8.0, backend: str = "auto") -> torch.Tensor:
    """The deltas of a distribution box head (Generalized Focal Loss, section 3.2): logits (..., 4 * K), per side a
    softmax over K bins, out (..., 4) the expectations ``sum_i p_i v_i`` in the logits' dtype (fp32 arithmetic and one
    rounding; float64 logits compute in float64: the kernel's oracle).  On the GPU every row runs in
    ``box_dist.hip``; what it does not serve runs as this torch expression with one warning per form."""
    from . import native
    K = int(K)
    if K < 2 or logits.shape[-1] != 4 * K:
        raise ValueError("box_integral: logits (..., 4 * K) with K >= 2 expected, got {} with K = {}".format(
            tuple(logits.shape), K))
    if backend == "auto":
        backend = "hip" if (logits.is_cuda and native.available()) else "torch"
    if backend == "hip":
        try:
            return native.BoxIntegralFn.apply(logits, K, float(R))
        except native.NotServed:
            key = ("integral", K, logits.dtype)
            if key not in _FALLBACK_WARNED:
                _FALLBACK_WARNED.add(key)
                warnings.warn("box_dist.hip does not serve {} bins of {}: the box integral runs as the torch "
                              "expression".format(K, logits.dtype))
    return _box_integral_torch(logits, K, float(R))


def clip_boxes(boxes: torch.Tensor, height: float, width: float) -> torch.Tensor:
    """Clamp x to [0, W] and y to [0, H] (0.4-era ClipBoxes bound, pinned by a unit test)."""
    x1 = boxes[..., 0].clamp(0, width)
    y1 = boxes[..., 1].clamp(0, height)
    x2 = boxes[..., 2].clamp(0, width)
    y2 = boxes[..., 3].clamp(0, height)
    return torch.stack([x1, y1, x2, y2], dim=-1)


def box_iou_plain(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """IoU without the +1 convention (tf.image.non_max_suppression semantics)."""
    area_a = (a[:, 2] - a[:, 0]).clamp_min(0) * (a[:, 3] - a[:, 1]).clamp_min(0)
    area_b = (b[:, 2] - b[:, 0]).clamp_min(0) * (b[:, 3] - b[:, 1]).clamp_min(0)
    lt = torch.maximum(a[:, None, :2], b[None, :, :2])
    rb = torch.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp_min(0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a[:, None] + area_b[None, :] - inter
    return torch.where(union > 0, inter / union, torch.zeros_like(inter))


def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float, max_output: int) -> torch.Tensor:
    """Greedy NMS, keeps indices in decreasing-score order (TF semantics: suppress if IoU > thr)."""
    if boxes.numel() == 0:
        return torch.zeros((0,), dtype=torch.long, device=boxes.device)
    order = torch.argsort(scores, descending=True, stable=True)
    b = boxes[order]
    iou = box_iou_plain(b, b)
    n = b.shape[0]
    suppressed = torch.zeros(n, dtype=torch.bool, device=boxes.device)
    keep = []
    iou_cpu = iou.cpu()
    sup = suppressed.cpu()
    for i in range(n):
        if sup[i]:
            continue
        keep.append(i)
        if len(keep) >= max_output:
            break
        sup |= iou_cpu[i] > iou_threshold
    return order[torch.tensor(keep, dtype=torch.long, device=boxes.device)]


SOFT_NMS_KINDS = ("linear", "gaussian")


def check_nms_kind(nms_kind: str, sigma: float, min_score: Optional[float], score_threshold: float) -> float:
    """Validate ``(nms_kind, sigma, min_score)``; returns the score floor (``score_threshold`` when none is given)."""
    if nms_kind not in ("hard",) + SOFT_NMS_KINDS:
        raise ValueError("nms_kind must be hard, linear or gaussian, got {!r}".format(nms_kind))
    floor = float(score_threshold if min_score is None else min_score)
    if nms_kind != "hard" and not float(sigma) > 0:
        raise ValueError("soft_nms_sigma must be > 0, got {}".format(sigma))
    if nms_kind != "hard" and floor < 0:
        raise ValueError("soft_nms_min_score must be >= 0, got {}".format(floor))
    return floor


def soft_nms(boxes: torch.Tensor, scores: torch.Tensor, kind: str, iou_threshold: float = 0.5, sigma: float = 0.5,
             min_score: float = 0.05, max_output: int = 300) -> Tuple[torch.Tensor, torch.Tensor]:
    """Soft-NMS (Bodla et al., ICCV 2017) of one (image, class) segment, in the dtype of ``boxes`` / ``scores``: fp32 is
    the CPU path and the fallback, float64 the oracle of ``csrc/kernels/soft_nms.hip``.

    Until ``max_output`` boxes are emitted: pick the live candidate of largest current score (an exact tie goes to the
    lower index); stop if that score ``<= min_score``; emit it and mark it dead; multiply every other live score by
    ``w(u)``, ``u`` its IoU (:func:`box_iou_plain`) with the pick -- ``linear``: ``1 - u`` where ``u > iou_threshold``,
    else exactly 1; ``gaussian``: ``exp(-(u * u) / sigma)`` -- and a score that falls to ``<= min_score`` is dead from
    then on.  Returns (indices into ``boxes`` in emission order, their decayed scores)."""
    if kind not in SOFT_NMS_KINDS:
        raise ValueError("soft_nms: kind must be linear or gaussian, got {!r}".format(kind))
    check_nms_kind(kind, sigma, min_score, min_score)
    s = scores.clone()             # a dead candidate has score 0
    zero = torch.zeros_like(s)
    idx, out = [], []
    for _ in range(min(int(max_output), s.numel())):
        i = int(torch.argmax(s))    # the first maximal value: the lower index on a tie
        top = s[i]
        if not bool(top > min_score):
            break
        idx.append(i)
        out.append(top)
        u = box_iou_plain(boxes[i:i + 1], boxes)[0]
        if kind == "linear":
            w = torch.where(u > iou_threshold, 1 - u, torch.ones_like(u))
        else:
            w = torch.exp(-(u * u) / sigma)
        s = s * w
        s[i] = 0
        s = torch.where(s > min_score, s, zero)
    if not idx:
        return torch.zeros(0, dtype=torch.long, device=boxes.device), scores.new_zeros(0)
    return torch.tensor(idx, dtype=torch.long, device=boxes.device), torch.stack(out)


def filter_detections(boxes: torch.Tensor, classification: torch.Tensor, nms_enabled: bool = True,
                      class_specific_filter: bool = True, nms_threshold: float = 0.5,
                      score_threshold: float = 0.05, max_detections: int = 300,
                      backend: Optional[str] = None, nms_kind: str = "hard", soft_nms_sigma: float = 0.5,
                      soft_nms_min_score: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-image FilterDetections.  boxes (A, 4), classification (A, C) probabilities.

    ``nms_kind`` linear / gaussian replaces the greedy NMS by :func:`soft_nms` (torch on every backend here; the
    device form is ``native.filter_detections_batched``) and ranks across classes by the decayed scores.

    Returns boxes (max_det, 4), scores (max_det,), labels (max_det,) padded with -1.
    """
    from . import native  # local import: avoids a cycle at package import
    if backend is None:
        backend = "hip" if (boxes.is_cuda and native.available()) else "torch"
    dev = boxes.device
    floor = check_nms_kind(nms_kind, soft_nms_sigma, soft_nms_min_score, score_threshold)
    all_idx, all_lab, all_sc = [], [], None      # all_sc: the decayed scores of a soft kind
    if nms_kind != "hard" and nms_enabled:
        if class_specific_filter:
            segments = [(classification[:, c], c) for c in range(classification.shape[1])]
        else:
            segments = [classification.max(dim=1)]
        all_sc = []
        for s, lab in segments:
            idx = torch.nonzero(s > score_threshold).flatten()
            k, sc = soft_nms(boxes[idx], s[idx], nms_kind, nms_threshold, soft_nms_sigma, floor, max_detections)
            all_idx.append(idx[k])
            all_sc.append(sc)
            all_lab.append(lab[idx[k]] if torch.is_tensor(lab) else torch.full_like(k, lab))
    elif class_specific_filter:
        C = classification.shape[1]
        for c in range(C):
            s = classification[:, c]
            idx = torch.nonzero(s > score_threshold).flatten()
            if idx.numel() == 0:
                continue
            if nms_enabled:
                if backend == "hip":
                    k = native.nms(boxes[idx].float().contiguous(), s[idx].float().contiguous(), nms_threshold, max_detections)
                else:
                    k = nms(boxes[idx], s[idx], nms_threshold, max_detections)
                idx = idx[k]
            all_idx.append(idx)
            all_lab.append(torch.full_like(idx, c))
    else:
        s, lab = classification.max(dim=1)
        idx = torch.nonzero(s > score_threshold).flatten()
        if nms_enabled and idx.numel():
            k = nms(boxes[idx], s[idx], nms_threshold, max_detections)
            idx = idx[k]
        all_idx.append(idx)
        all_lab.append(lab[idx])
    out_b = torch.full((max_detections, 4), -1.0, device=dev)
    out_s = torch.full((max_detections,), -1.0, device=dev)
    out_l = torch.full((max_detections,), -1, dtype=torch.int32, device=dev)
    if all_idx:
        idx = torch.cat(all_idx)
        lab = torch.cat(all_lab)
        if idx.numel():
            sc = classification[idx, lab] if all_sc is None else torch.cat(all_sc)
            k = min(max_detections, sc.numel())
            top_s, top_i = torch.topk(sc, k)
            out_b[:k] = boxes[idx[top_i]].float()
            out_s[:k] = top_s.float()
            out_l[:k] = lab[top_i].to(torch.int32)
    return out_b, out_s, out_l

