"""Anchor generation and anchor-target assignment.

Behavioural spec: keras-retinanet ``utils.anchors`` as imported by the reference at
``/root/reference/train.py:51`` (``anchor_targets_bbox``, ``make_shapes_callback``) and used
implicitly by every generator built at ``train.py:197-293``.  SURVEY §2.8.4-2.8.5.

Two implementations live here:

* a float64 numpy *oracle* (``anchor_targets_bbox``) that reproduces the reference
  semantics literally (IoU with the "+1 pixel" convention, 0.4/0.5 thresholds,
  outside-centre ignore, corner-offset regression with std 0.2);
* a batched torch implementation (``anchor_targets_torch``) that runs on the GPU (or CPU)
  with compact outputs -- per-anchor ``state`` (-1 ignore / 0 negative / 1 positive),
  ``label`` (class id of the matched box) and ``regression`` (A, 4) -- instead of the
  reference's 65 MB/image one-hot tensor.  The fused HIP kernel in
  ``csrc/kernels/targets.hip`` implements the same contract.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch


@dataclass
class AnchorParameters:
    """Anchor configuration (keras-retinanet ``AnchorParameters.default``)."""

    sizes: Sequence[float] = (32, 64, 128, 256, 512)
    strides: Sequence[int] = (8, 16, 32, 64, 128)
    ratios: Sequence[float] = (0.5, 1.0, 2.0)
    scales: Sequence[float] = (2.0 ** 0.0, 2.0 ** (1.0 / 3.0), 2.0 ** (2.0 / 3.0))

    def num_anchors(self) -> int:
        return len(self.ratios) * len(self.scales)


AnchorParameters.default = AnchorParameters()  # type: ignore[attr-defined]

PYRAMID_LEVELS = (3, 4, 5, 6, 7)
BOX_STD = 0.2
BOX_MEAN = 0.0
POSITIVE_OVERLAP = 0.5
NEGATIVE_OVERLAP = 0.4


def generate_anchors(base_size: float = 16, ratios=None, scales=None) -> np.ndarray:
    """Reference anchors (centred at the origin) for one pyramid level.

    Ordering is ratio-major, scale-minor, which is also the channel ordering of the
    regression/classification heads.
    """
    ratios = np.asarray(AnchorParameters.default.ratios if ratios is None else ratios, dtype=np.float64)
    scales = np.asarray(AnchorParameters.default.scales if scales is None else scales, dtype=np.float64)
    rr = np.repeat(ratios, len(scales))          # ratio for anchor i
    ss = np.tile(scales, len(ratios))            # scale for anchor i
    side = base_size * ss
    area = side * side
    w = np.sqrt(area / rr)
    h = w * rr
    out = np.stack([-0.5 * w, -0.5 * h, 0.5 * w, 0.5 * h], axis=1)
    return out


def shift(shape: Tuple[int, int], stride: int, anchors: np.ndarray) -> np.ndarray:
    """Tile ``anchors`` over a (H, W) feature map; centres at (i + 0.5) * stride.

    Result is (H*W*A, 4), position-major (row-major over y then x), anchor-minor.
    """
    h, w = int(shape[0]), int(shape[1])
    sx = (np.arange(w, dtype=np.float64) + 0.5) * stride
    sy = (np.arange(h, dtype=np.float64) + 0.5) * stride
    gx, gy = np.meshgrid(sx, sy)
    shifts = np.stack([gx.ravel(), gy.ravel(), gx.ravel(), gy.ravel()], axis=1)
    return (shifts[:, None, :] + anchors[None, :, :]).reshape(-1, 4)


def guess_shapes(image_shape: Sequence[int], pyramid_levels=PYRAMID_LEVELS) -> List[Tuple[int, int]]:
    """Closed-form feature-map shapes for the ResNet backbone: ceil(size / 2**level)."""
    h, w = int(image_shape[0]), int(image_shape[1])
    return [((h + 2 ** x - 1) // (2 ** x), (w + 2 ** x - 1) // (2 ** x)) for x in pyramid_levels]


def anchors_for_shape(image_shape: Sequence[int], pyramid_levels=PYRAMID_LEVELS,
                      anchor_params: Optional[AnchorParameters] = None,
                      shapes_callback=None) -> np.ndarray:
    """All anchors (float64) for an input image of ``image_shape`` (H, W[, C])."""
    p = anchor_params or AnchorParameters.default
    shapes = (shapes_callback or guess_shapes)(image_shape[:2], pyramid_levels)
    out = []
    for idx, lvl in enumerate(pyramid_levels):
        base = generate_anchors(p.sizes[idx], p.ratios, p.scales)
        out.append(shift(shapes[idx], p.strides[idx], base))
    return np.concatenate(out, axis=0)


def level_sizes(image_shape, pyramid_levels=PYRAMID_LEVELS) -> List[int]:
    """Number of anchors on each pyramid level."""
    A = AnchorParameters.default.num_anchors()
    return [h * w * A for (h, w) in guess_shapes(image_shape, pyramid_levels)]


def make_shapes_callback(model):
    """Shape oracle that measures the real feature-map shapes of ``model``.

    The reference swaps this in for vgg/densenet backbones (``train.py:428-432``).
    ``model`` must expose ``pyramid_shapes(image_shape)``.
    """
    def get_shapes(image_shape, pyramid_levels=PYRAMID_LEVELS):
        return model.pyramid_shapes(tuple(image_shape[:2]))
    return get_shapes


# ----------------------------------------------------------------------------------------
# numpy oracle
# ----------------------------------------------------------------------------------------

def compute_overlap(boxes: np.ndarray, query_boxes: np.ndarray) -> np.ndarray:
    """IoU matrix (N, K) with the reference's "+1 pixel" convention.

    Replaces the Cython ``compute_overlap.pyx``; the native C++ version lives in
    ``csrc/cpu/boxes_cpu.cpp`` and is used when the CPU extension is built.
    """
    boxes = np.asarray(boxes, dtype=np.float64)
    q = np.asarray(query_boxes, dtype=np.float64)
    if q.shape[0] == 0 or boxes.shape[0] == 0:
        return np.zeros((boxes.shape[0], q.shape[0]), dtype=np.float64)
    area_q = (q[:, 2] - q[:, 0] + 1) * (q[:, 3] - q[:, 1] + 1)
    iw = np.minimum(boxes[:, None, 2], q[None, :, 2]) - np.maximum(boxes[:, None, 0], q[None, :, 0]) + 1
    ih = np.minimum(boxes[:, None, 3], q[None, :, 3]) - np.maximum(boxes[:, None, 1], q[None, :, 1]) + 1
    iw = np.clip(iw, 0, None)
    ih = np.clip(ih, 0, None)
    inter = iw * ih
    ua = (boxes[:, None, 2] - boxes[:, None, 0] + 1) * (boxes[:, None, 3] - boxes[:, None, 1] + 1) + area_q[None, :] - inter
    out = np.where((iw > 0) & (ih > 0), inter / ua, 0.0)
    return out


def bbox_transform(anchors: np.ndarray, gt_boxes: np.ndarray, mean=BOX_MEAN, std=BOX_STD) -> np.ndarray:
    """Corner-offset regression targets normalised by anchor width/height."""
    aw = anchors[:, 2] - anchors[:, 0]
    ah = anchors[:, 3] - anchors[:, 1]
    t = np.stack([(gt_boxes[:, 0] - anchors[:, 0]) / aw,
                  (gt_boxes[:, 1] - anchors[:, 1]) / ah,
                  (gt_boxes[:, 2] - anchors[:, 2]) / aw,
                  (gt_boxes[:, 3] - anchors[:, 3]) / ah], axis=1)
    return (t - mean) / std


def anchor_targets_bbox(image_shape, annotations: np.ndarray, num_classes: int, mask_shape=None,
                        negative_overlap=NEGATIVE_OVERLAP, positive_overlap=POSITIVE_OVERLAP,
                        shapes_callback=None, anchors: Optional[np.ndarray] = None):
    """Reference-semantics targets for one image.

    Returns ``(labels (A, C) with -1 rows for ignore, regression (A, 4), state (A,))``.
    """
    if anchors is None:
        anchors = anchors_for_shape(image_shape, shapes_callback=shapes_callback)
    A = anchors.shape[0]
    annotations = np.asarray(annotations, dtype=np.float64).reshape(-1, 5)
    labels = np.full((A, num_classes), -1.0)
    state = np.full((A,), -1.0)
    if annotations.shape[0]:
        overlaps = compute_overlap(anchors, annotations[:, :4])
        arg = np.argmax(overlaps, axis=1)
        mx = overlaps[np.arange(A), arg]
        neg = mx < negative_overlap
        labels[neg, :] = 0
        state[neg] = 0
        matched = annotations[arg]
        pos = mx >= positive_overlap
        labels[pos, :] = 0
        labels[pos, matched[pos, 4].astype(int)] = 1
        state[pos] = 1
    else:
        labels[:] = 0
        state[:] = 0
        matched = np.zeros((A, 5))
        matched[:, :4] = anchors
    mh, mw = (image_shape if mask_shape is None else mask_shape)[:2]
    cx = (anchors[:, 0] + anchors[:, 2]) / 2
    cy = (anchors[:, 1] + anchors[:, 3]) / 2
    outside = (cx >= mw) | (cy >= mh)
    labels[outside, :] = -1
    state[outside] = -1
    regression = bbox_transform(anchors, matched[:, :4])
    return labels, regression, state


# ----------------------------------------------------------------------------------------
# batched torch implementation (device-resident targets)
# ----------------------------------------------------------------------------------------

def centers_round_down(anchors64: np.ndarray) -> np.ndarray:
    """Anchor centres (A, 2) as the largest float32 <= the float64 centre.

    The reference tests ``cx >= W`` in float64; rounding the centre DOWN to float32 keeps every
    comparison against an integer image size identical (e.g. 95.99999999999999 must not become 96).
    """
    c64 = np.stack([(anchors64[:, 0] + anchors64[:, 2]) / 2, (anchors64[:, 1] + anchors64[:, 3]) / 2], axis=1)
    c32 = c64.astype(np.float32)
    up = c32.astype(np.float64) > c64
    c32[up] = np.nextafter(c32[up], np.float32(-np.inf))
    return c32


class AnchorCache:
    """Per-(padded shape, device) cache of anchors (float32 (A, 4)) and their centres (A, 2)."""

    def __init__(self, anchor_params: Optional[AnchorParameters] = None):
        self.p = anchor_params or AnchorParameters.default
        self._cache = {}

    def _entry(self, image_shape, device, shapes_callback):
        key = (int(image_shape[0]), int(image_shape[1]), str(device))
        t = self._cache.get(key)
        if t is None:
            a = anchors_for_shape(image_shape, anchor_params=self.p, shapes_callback=shapes_callback)
            t = (torch.from_numpy(a.astype(np.float32)).to(device),
                 torch.from_numpy(centers_round_down(a)).to(device))
            self._cache[key] = t
        return t

    def get(self, image_shape, device, shapes_callback=None) -> torch.Tensor:
        return self._entry(image_shape, device, shapes_callback)[0]

    def centers(self, image_shape, device, shapes_callback=None) -> torch.Tensor:
        return self._entry(image_shape, device, shapes_callback)[1]

    def levels(self, image_shape, device=None, shapes_callback=None) -> np.ndarray:
        """The level table of the padded shape, (L, 4) int64 rows ``(first anchor index, h, w, stride)``: host
        values (the ATSS kernels take them by value), the same for every device."""
        key = (int(image_shape[0]), int(image_shape[1]), "levels")
        t = self._cache.get(key)
        if t is None:
            t = level_table(image_shape, shapes_callback, anchor_params=self.p)
            t.setflags(write=False)
            self._cache[key] = t
        return t


def anchor_targets_torch(anchors: torch.Tensor, gt: torch.Tensor, gt_count: torch.Tensor,
                         mask_hw: torch.Tensor,
                         negative_overlap=NEGATIVE_OVERLAP, positive_overlap=POSITIVE_OVERLAP,
                         centers: Optional[torch.Tensor] = None):
    """Batched targets.

    Args:
      anchors: (A, 4) float32.
      gt: (B, G, 5) float32 padded boxes ``[x1, y1, x2, y2, label]``; rows >= gt_count ignored.
      gt_count: (B,) int number of valid boxes per image.
      mask_hw: (B, 2) unpadded image (H, W) per image.
    Returns:
      state (B, A) int8, label (B, A) int32, regression (B, A, 4) float32.
    """
    B, G = gt.shape[0], gt.shape[1]
    A = anchors.shape[0]
    dev = anchors.device
    ax1, ay1, ax2, ay2 = anchors.unbind(-1)
    if G > 0:
        g = gt[..., :4]
        gx1, gy1, gx2, gy2 = [g[..., i][:, None, :] for i in range(4)]  # (B,1,G)
        iw = (torch.minimum(ax2[None, :, None], gx2) - torch.maximum(ax1[None, :, None], gx1) + 1).clamp_min(0)
        ih = (torch.minimum(ay2[None, :, None], gy2) - torch.maximum(ay1[None, :, None], gy1) + 1).clamp_min(0)
        inter = iw * ih
        area_a = ((ax2 - ax1 + 1) * (ay2 - ay1 + 1))[None, :, None]
        area_g = ((gx2 - gx1 + 1) * (gy2 - gy1 + 1))
        iou = inter / (area_a + area_g - inter)
        valid = torch.arange(G, device=dev)[None, None, :] < gt_count.to(dev)[:, None, None]
        iou = torch.where(valid, iou, torch.full_like(iou, -1.0))
        mx, arg = iou.max(dim=2)                      # first max wins, like np.argmax
        has = (gt_count.to(dev) > 0)[:, None]
        mx = torch.where(has, mx, torch.zeros_like(mx))
        state = torch.full((B, A), -1, dtype=torch.int8, device=dev)
        state = torch.where(mx < negative_overlap, torch.zeros_like(state), state)
        state = torch.where(mx >= positive_overlap, torch.ones_like(state), state)
        matched = torch.gather(gt, 1, arg[..., None].expand(B, A, 5))
        matched = torch.where(has[..., None], matched,
                              torch.cat([anchors, torch.zeros_like(anchors[:, :1])], 1)[None].expand(B, A, 5))
        label = matched[..., 4].to(torch.int32)
        mbox = matched[..., :4]
    else:
        state = torch.zeros((B, A), dtype=torch.int8, device=dev)
        label = torch.zeros((B, A), dtype=torch.int32, device=dev)
        mbox = anchors[None].expand(B, A, 4)
    if centers is None:
        centers = torch.from_numpy(centers_round_down(anchors.double().cpu().numpy())).to(dev)
    cx, cy = centers[:, 0], centers[:, 1]
    mh = mask_hw[:, 0].to(dev).to(anchors.dtype)[:, None]
    mw = mask_hw[:, 1].to(dev).to(anchors.dtype)[:, None]
    outside = (cx[None] >= mw) | (cy[None] >= mh)
    state = torch.where(outside, torch.full_like(state, -1), state)
    aw = (ax2 - ax1)[None]
    ah = (ay2 - ay1)[None]
    reg = torch.stack([(mbox[..., 0] - ax1[None]) / aw, (mbox[..., 1] - ay1[None]) / ah,
                       (mbox[..., 2] - ax2[None]) / aw, (mbox[..., 3] - ay2[None]) / ah], -1)
    reg = (reg - BOX_MEAN) / BOX_STD
    return state, label, reg


# ----------------------------------------------------------------------------------------
# ATSS (Zhang et al., CVPR 2020, Algorithm 1): per-box thresholds from the nearest anchors
# ----------------------------------------------------------------------------------------
ATSS_TOPK = 9
ATSS_MAX_TOPK = 16
ATSS_INSIDE_EPS = 0.01
ATSS_WINDOW = 4         # half-size, in cells, of the window the HIP kernel scans around the box centre's cell


def level_table(image_shape, shapes_callback=None, anchor_params: Optional[AnchorParameters] = None,
                pyramid_levels=PYRAMID_LEVELS) -> np.ndarray:
    """(L, 4) int64 rows ``(first anchor index, h, w, stride)`` of the padded shape, as ``anchors_for_shape`` lays the
    levels out."""
    p = anchor_params or AnchorParameters.default
    shapes = (shapes_callback or guess_shapes)(image_shape[:2], pyramid_levels)
    rows, first = [], 0
    for idx in range(len(pyramid_levels)):
        h, w = int(shapes[idx][0]), int(shapes[idx][1])
        rows.append((first, h, w, int(p.strides[idx])))
        first += h * w * p.num_anchors()
    return np.asarray(rows, dtype=np.int64)


def _check_topk(topk) -> int:
    if int(topk) != topk or not 1 <= int(topk) <= ATSS_MAX_TOPK:
        raise ValueError("topk must be an integer in 1..{}, got {!r}".format(ATSS_MAX_TOPK, topk))
    return int(topk)


def _check_levels(levels, A: int) -> Tuple[np.ndarray, int]:
    """The level table as (L, 4) int64 and the anchors per location; a table that does not tile ``A`` is refused."""
    lv = np.asarray(levels, dtype=np.int64).reshape(-1, 4)
    locs = int((lv[:, 1] * lv[:, 2]).sum())
    if lv.shape[0] == 0 or (lv[:, 1:] <= 0).any() or locs == 0 or A % locs:
        raise ValueError("the level table {} does not add up to {} anchors".format(lv.tolist(), A))
    A0 = A // locs
    first = np.concatenate([[0], np.cumsum(lv[:, 1] * lv[:, 2] * A0)[:-1]])
    if (lv[:, 0] != first).any():
        raise ValueError("the level table {} does not add up to {} anchors".format(lv.tolist(), A))
    return lv, A0


def atss_window(h: int, w: int, stride: int, gcx: float, gcy: float, topk: int) -> Tuple[int, int, int, int]:
    """The rectangle of locations ``(x0, x1, y0, y1)``, inclusive, in which the HIP kernel looks for the ``topk``
    locations nearest to ``(gcx, gcy)``; this is that rule in Python.

    The window is ATSS_WINDOW cells around the cell the point falls into, clipped to the grid.  A location outside it
    is more than ATSS_WINDOW cells from that cell on one axis, and the point is at most half a cell from the cell's
    centre on that axis (further only towards the grid's outside), so the location is at least ATSS_WINDOW + 0.5
    strides away.  When the window holds ``topk`` locations closer than ATSS_WINDOW strides (half a stride of slack:
    fp32 rounding is far below it), they beat every location outside it; otherwise the whole level is scanned."""
    f32 = np.float32
    R = ATSS_WINDOW
    ix0 = min(max(int(math.floor(f32(gcx) / f32(stride))), 0), w - 1)
    iy0 = min(max(int(math.floor(f32(gcy) / f32(stride))), 0), h - 1)
    x0, x1, y0, y1 = max(ix0 - R, 0), min(ix0 + R, w - 1), max(iy0 - R, 0), min(iy0 + R, h - 1)
    if x0 == 0 and y0 == 0 and x1 == w - 1 and y1 == h - 1:
        return x0, x1, y0, y1
    dx = (np.arange(x0, x1 + 1, dtype=f32) + f32(0.5)) * f32(stride) - f32(gcx)
    dy = (np.arange(y0, y1 + 1, dtype=f32) + f32(0.5)) * f32(stride) - f32(gcy)
    d2 = (dx * dx)[None, :] + (dy * dy)[:, None]
    if int((d2 < f32(R * stride) * f32(R * stride)).sum()) >= min(topk, h * w):
        return x0, x1, y0, y1
    return 0, w - 1, 0, h - 1


def _nearest_locations(h, w, stride, gcx, gcy, k, rect=None, dtype=np.float64) -> np.ndarray:
    """The ``min(k, h * w)`` row-major location indices nearest to (gcx, gcy), ordered by (d2, index); brute force
    over the level, or over ``rect`` = (x0, x1, y0, y1)."""
    x0, x1, y0, y1 = rect or (0, w - 1, 0, h - 1)
    t = dtype
    dx = (np.arange(x0, x1 + 1).astype(t) + t(0.5)) * t(stride) - t(gcx)
    dy = (np.arange(y0, y1 + 1).astype(t) + t(0.5)) * t(stride) - t(gcy)
    d2 = ((dx * dx)[None, :] + (dy * dy)[:, None]).ravel()
    idx = (np.arange(y0, y1 + 1)[:, None] * w + np.arange(x0, x1 + 1)[None, :]).ravel()
    order = np.lexsort((idx, d2))
    return idx[order[:min(k, h * w)]]


def atss_assign(anchors: np.ndarray, levels, boxes: np.ndarray, topk: int = ATSS_TOPK) -> dict:
    """ATSS for one image in float64, brute force: the specification of the HIP kernels and the torch form.

    ``boxes`` (n, 4+).  Returns ``arg`` (A,) the box of every anchor or -1, ``best`` (A,) its IoU or -1,
    ``threshold`` (n,), ``selected`` (n, L, topk) location indices per level in selection order (-1 padded),
    ``candidates`` (n, N) anchor indices, ``iou`` (n, N) their IoU with the box and ``inside`` (n, N) whether their
    grid centre lies inside it."""
    topk = _check_topk(topk)
    anchors = np.asarray(anchors, dtype=np.float64)
    A = anchors.shape[0]
    lv, A0 = _check_levels(levels, A)
    boxes = np.asarray(boxes, dtype=np.float64)
    boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.ndim > 1 else 4)
    n, L = boxes.shape[0], lv.shape[0]
    N = int(sum(min(topk, h * w) for _, h, w, _ in lv) * A0)
    out = {"arg": np.full(A, -1, dtype=np.int64), "best": np.full(A, -1.0), "threshold": np.zeros(n),
           "selected": np.full((n, L, topk), -1, dtype=np.int64), "candidates": np.zeros((n, N), dtype=np.int64),
           "iou": np.zeros((n, N)), "inside": np.zeros((n, N), dtype=bool)}
    for g in range(n):
        x1, y1, x2, y2 = boxes[g, :4]
        gcx, gcy = (x1 + x2) / 2, (y1 + y2) / 2
        cand, ccx, ccy = [], [], []
        for l, (first, h, w, stride) in enumerate(lv):
            loc = _nearest_locations(h, w, stride, gcx, gcy, topk)
            out["selected"][g, l, :len(loc)] = loc
            cand.append((first + loc[:, None] * A0 + np.arange(A0)[None, :]).ravel())
            ccx.append(np.repeat((loc % w + 0.5) * stride, A0))
            ccy.append(np.repeat((loc // w + 0.5) * stride, A0))
        cand, ccx, ccy = np.concatenate(cand), np.concatenate(ccx), np.concatenate(ccy)
        iou = compute_overlap(anchors[cand], boxes[g:g + 1, :4])[:, 0]
        thr = iou.mean() + (iou.std(ddof=1) if iou.size > 1 else 0.0)
        inside = np.minimum(np.minimum(ccx - x1, ccy - y1), np.minimum(x2 - ccx, y2 - ccy)) > ATSS_INSIDE_EPS
        take = inside & (iou >= thr) & (iou > out["best"][cand])          # strict: the lower box index keeps a tie
        out["best"][cand[take]] = iou[take]
        out["arg"][cand[take]] = g
        out["threshold"][g] = thr
        out["candidates"][g] = cand
        out["iou"][g] = iou
        out["inside"][g] = inside
    return out


def atss_targets_bbox(image_shape, annotations: np.ndarray, num_classes: int, mask_shape=None, topk: int = ATSS_TOPK,
                      shapes_callback=None, anchors: Optional[np.ndarray] = None):
    """ATSS targets for one image, the float64 oracle; returns like ``anchor_targets_bbox``:
    ``(labels (A, C) with -1 rows for ignore, regression (A, 4), state (A,))``.

    Every box takes, on every level, the ``min(topk, h * w)`` locations whose grid centre is nearest to its own
    (ties to the lower index) and all anchors there as candidates; its threshold is mean + unbiased std of their
    IoUs; a candidate at or above it whose grid centre lies inside the box is positive, for the box of largest IoU
    when for several (ties to the lower box).  Everything else is negative with a zero regression target -- there is
    no ignore band -- except that anchors centred outside the image are ignored, positives included."""
    if anchors is None:
        anchors = anchors_for_shape(image_shape, shapes_callback=shapes_callback)
    anchors = np.asarray(anchors, dtype=np.float64)
    A = anchors.shape[0]
    annotations = np.asarray(annotations, dtype=np.float64).reshape(-1, 5)
    r = atss_assign(anchors, level_table(image_shape, shapes_callback), annotations, topk)
    pos = r["arg"] >= 0
    labels = np.zeros((A, num_classes))
    state = np.zeros((A,))
    regression = np.zeros((A, 4))
    if pos.any():
        matched = annotations[r["arg"][pos]]
        labels[np.nonzero(pos)[0], matched[:, 4].astype(int)] = 1
        state[pos] = 1
        regression[pos] = bbox_transform(anchors[pos], matched[:, :4])
    mh, mw = (image_shape if mask_shape is None else mask_shape)[:2]
    cx = (anchors[:, 0] + anchors[:, 2]) / 2
    cy = (anchors[:, 1] + anchors[:, 3]) / 2
    outside = (cx >= mw) | (cy >= mh)
    labels[outside, :] = -1
    state[outside] = -1
    return labels, regression, state


def atss_targets_torch(anchors: torch.Tensor, levels, gt: torch.Tensor, gt_count: torch.Tensor,
                       mask_hw: torch.Tensor, topk: int = ATSS_TOPK, centers: Optional[torch.Tensor] = None,
                       return_aux: bool = False):
    """Batched fp32 ATSS targets (CPU devices and ``target_backend="torch"``); arguments and results as
    ``anchor_targets_torch`` plus the level table.  With ``return_aux`` also ``(threshold (B, G), selected
    (B, G, L, topk) int32 location indices, -1 padded)``; rows at or beyond ``gt_count`` hold inf and -1.

    The distances are computed as the HIP kernel computes them -- every product and sum rounded to fp32 on its own
    -- so both select the same locations bit for bit; nothing here depends on the data in shape or control flow."""
    topk = _check_topk(topk)
    B, G = gt.shape[0], gt.shape[1]
    A = anchors.shape[0]
    dev = anchors.device
    lv, A0 = _check_levels(levels, A)
    L = lv.shape[0]
    f32 = torch.float32
    gt = gt.to(f32)
    cnt = gt_count.to(dev).to(torch.int64)
    valid = torch.arange(G, device=dev)[None, :] < cnt[:, None]                    # (B, G)
    # rows past the count may hold anything: they are replaced before any arithmetic
    box = torch.where(valid[..., None], gt[..., :4], torch.zeros((), dtype=f32, device=dev))
    x1, y1, x2, y2 = box.unbind(-1)
    gcx, gcy = (x1 + x2) * 0.5, (y1 + y2) * 0.5
    sel = torch.full((B, G, L, topk), -1, dtype=torch.int32, device=dev)
    cand, ccx, ccy = [], [], []
    for l, (first, h, w, stride) in enumerate(lv.tolist()):
        k = min(topk, h * w)
        dx = ((torch.arange(w, device=dev, dtype=f32) + 0.5) * float(stride))[None, None, None, :] - gcx[..., None, None]
        dy = ((torch.arange(h, device=dev, dtype=f32) + 0.5) * float(stride))[None, None, :, None] - gcy[..., None, None]
        d2 = ((dx * dx) + (dy * dy)).reshape(B, G, h * w)
        loc = torch.sort(d2, dim=-1, stable=True)[1][..., :k]                      # (d2, index) order
        sel[:, :, l, :k] = loc.to(torch.int32)
        cand.append((first + loc[..., None] * A0 + torch.arange(A0, device=dev)).reshape(B, G, k * A0))
        ccx.append((((loc % w).to(f32) + 0.5) * float(stride)).repeat_interleave(A0, dim=-1))
        ccy.append(((torch.div(loc, w, rounding_mode="floor").to(f32) + 0.5) * float(stride))
                   .repeat_interleave(A0, dim=-1))
    cand, ccx, ccy = torch.cat(cand, -1), torch.cat(ccx, -1), torch.cat(ccy, -1)  # (B, G, N)
    N = cand.shape[-1]
    ca = anchors[cand]                                                             # (B, G, N, 4)
    ax1, ay1, ax2, ay2 = ca.unbind(-1)
    gx1, gy1, gx2, gy2 = x1[..., None], y1[..., None], x2[..., None], y2[..., None]
    iw = torch.minimum(ax2, gx2) - torch.maximum(ax1, gx1) + 1
    ih = torch.minimum(ay2, gy2) - torch.maximum(ay1, gy1) + 1
    inter = iw * ih
    ua = (ax2 - ax1 + 1) * (ay2 - ay1 + 1) + (gx2 - gx1 + 1) * (gy2 - gy1 + 1) - inter
    iou = torch.where((iw > 0) & (ih > 0), inter / ua, torch.zeros_like(inter))
    mean = iou.sum(-1, keepdim=True) / N
    dev2 = ((iou - mean) * (iou - mean)).sum(-1, keepdim=True)
    thr = mean + (torch.sqrt(dev2 / (N - 1)) if N > 1 else torch.zeros_like(mean))  # (B, G, 1)
    inside = torch.minimum(torch.minimum(ccx - gx1, ccy - gy1), torch.minimum(gx2 - ccx, gy2 - ccy)) > ATSS_INSIDE_EPS
    pos = inside & (iou >= thr) & valid[..., None]
    # per anchor: the largest IoU among the boxes it is positive for, then the lowest such box
    key = (torch.arange(B, device=dev)[:, None, None] * A + cand).reshape(-1)
    score = torch.where(pos, iou, torch.full_like(iou, -1.0)).reshape(-1)
    best = torch.full((B * A,), -1.0, dtype=f32, device=dev).scatter_reduce(0, key, score, "amax", include_self=True)
    won = pos.reshape(-1) & (score == best[key])
    gidx = torch.arange(G, device=dev)[None, :, None].expand(B, G, N).reshape(-1)
    arg = torch.full((B * A,), G, dtype=torch.int64, device=dev).scatter_reduce(
        0, key, torch.where(won, gidx, torch.full_like(gidx, G)), "amin", include_self=True).reshape(B, A)
    is_pos = arg < G
    if G > 0:
        matched = torch.gather(gt, 1, arg.clamp(max=G - 1)[..., None].expand(B, A, 5))
    else:
        matched = torch.zeros((B, A, 5), dtype=f32, device=dev)
    a1, b1, a2, b2 = anchors.unbind(-1)
    aw, ah = (a2 - a1)[None], (b2 - b1)[None]
    reg = torch.stack([(matched[..., 0] - a1[None]) / aw, (matched[..., 1] - b1[None]) / ah,
                       (matched[..., 2] - a2[None]) / aw, (matched[..., 3] - b2[None]) / ah], -1)
    reg = (reg - BOX_MEAN) / BOX_STD
    reg = torch.where(is_pos[..., None], reg, torch.zeros_like(reg))
    label = torch.where(is_pos, matched[..., 4].to(torch.int32), torch.zeros((), dtype=torch.int32, device=dev))
    state = is_pos.to(torch.int8)
    if centers is None:
        centers = torch.from_numpy(centers_round_down(anchors.double().cpu().numpy())).to(dev)
    mh = mask_hw[:, 0].to(dev).to(f32)[:, None]
    mw = mask_hw[:, 1].to(dev).to(f32)[:, None]
    outside = (centers[None, :, 0] >= mw) | (centers[None, :, 1] >= mh)
    state = torch.where(outside, torch.full_like(state, -1), state)
    if return_aux:
        thr = torch.where(valid, thr[..., 0], torch.full_like(thr[..., 0], float("inf")))
        sel = torch.where(valid[..., None, None], sel, torch.full_like(sel, -1))
        return state, label, reg, thr, sel
    return state, label, reg


# ----------------------------------------------------------------------------------------
# TAL (Feng et al., "TOOD", ICCV 2021, section 3.2): positives from the predictions
# ----------------------------------------------------------------------------------------
TAL_TOPK = 13
TAL_MAX_TOPK = ATSS_MAX_TOPK
TAL_BETA = 6            # t = s^1 u^6; no flags, as with QFL's beta
TAL_EPS = 1e-7


def _tal_centres(lv: np.ndarray, A0: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per anchor the grid centre of its location, from the level table: ``((ix + .5) * stride, (iy + .5) * stride)``."""
    cx, cy = [], []
    for first, h, w, stride in lv.tolist():
        loc = np.arange(h * w)
        cx.append(np.repeat((loc % w + 0.5) * stride, A0))
        cy.append(np.repeat((loc // w + 0.5) * stride, A0))
    return np.concatenate(cx), np.concatenate(cy)


def tal_assign(anchors: np.ndarray, levels, boxes: np.ndarray, cls_logits: np.ndarray, reg: np.ndarray,
               topk: int = TAL_TOPK) -> dict:
    """Task-aligned assignment for one image in float64, brute force: the specification of the torch form (and of
    device kernels, which do not exist yet).  ``boxes`` (n, 5) ``[x1, y1, x2, y2, label]``, ``cls_logits`` (A, C),
    ``reg`` (A, 4) deltas.

    Anchor i's predicted box is ``bbox_transform_inv`` (mean 0, std 0.2) of its deltas with the corners ordered;
    ``u_ij = inter / (area_p + area_g - inter + 1e-7)``; ``t_ij = sigmoid(x[i, label_j]) * u_ij^6`` (the power by
    multiplications).  i is a candidate of j when the grid centre of its location lies inside the box (ATSS's test)
    and ``u_ij > 0``; a box selects its ``min(topk, n_j)`` candidates of largest t, ordered by (t descending, anchor
    index ascending); an anchor selected by several boxes takes the box of largest u, the lowest index in a tie.  Per
    box, over the anchors it finally holds, ``tmax`` and ``umax``; a held anchor's quality is
    ``t / (tmax + 1e-7) * umax``.

    Returns ``arg`` (A,) the box of every anchor or -1, ``quality`` (A,), ``u`` / ``t`` / ``candidate`` / ``selected``
    (n, A), ``cutoff`` (n, 2) the t of the last selected and of the first not selected candidate (nan where there is
    none), ``count`` (n,) the candidates per box, ``tmax`` / ``umax`` (n,)."""
    topk = _check_topk(topk)
    anchors = np.asarray(anchors, dtype=np.float64)
    A = anchors.shape[0]
    lv, A0 = _check_levels(levels, A)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    x = np.asarray(cls_logits, dtype=np.float64)
    d = np.asarray(reg, dtype=np.float64)
    n = boxes.shape[0]
    aw, ah = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    qx1, qy1 = anchors[:, 0] + d[:, 0] * BOX_STD * aw, anchors[:, 1] + d[:, 1] * BOX_STD * ah
    qx2, qy2 = anchors[:, 2] + d[:, 2] * BOX_STD * aw, anchors[:, 3] + d[:, 3] * BOX_STD * ah
    px1, px2, py1, py2 = np.minimum(qx1, qx2), np.maximum(qx1, qx2), np.minimum(qy1, qy2), np.maximum(qy1, qy2)
    ccx, ccy = _tal_centres(lv, A0)
    out = {"arg": np.full(A, -1, dtype=np.int64), "quality": np.zeros(A), "u": np.zeros((n, A)), "t": np.zeros((n, A)),
           "candidate": np.zeros((n, A), dtype=bool), "selected": np.zeros((n, A), dtype=bool),
           "cutoff": np.full((n, 2), np.nan), "count": np.zeros(n, dtype=np.int64), "tmax": np.zeros(n),
           "umax": np.zeros(n)}
    best = np.zeros(A)
    idx = np.arange(A)
    for j in range(n):
        x1, y1, x2, y2 = boxes[j, :4]
        iw = np.clip(np.minimum(px2, x2) - np.maximum(px1, x1), 0, None)
        ih = np.clip(np.minimum(py2, y2) - np.maximum(py1, y1), 0, None)
        inter = iw * ih
        u = inter / ((px2 - px1) * (py2 - py1) + (x2 - x1) * (y2 - y1) - inter + TAL_EPS)
        with np.errstate(over="ignore"):                    # exp overflows to inf for a very negative logit: s = 0
            s = 1.0 / (1.0 + np.exp(-x[:, int(boxes[j, 4])]))
        u2 = u * u
        t = s * (u2 * u2 * u2)
        inside = np.minimum(np.minimum(ccx - x1, ccy - y1), np.minimum(x2 - ccx, y2 - ccy)) > ATSS_INSIDE_EPS
        cand = inside & (u > 0)
        c = idx[cand]
        order = c[np.lexsort((c, -t[c]))]                   # (t descending, index ascending)
        take = order[:topk]
        out["u"][j], out["t"][j], out["candidate"][j], out["count"][j] = u, t, cand, c.size
        out["selected"][j, take] = True
        if take.size:
            out["cutoff"][j, 0] = t[take[-1]]
        if order.size > topk:
            out["cutoff"][j, 1] = t[order[topk]]
        win = take[u[take] > best[take]]                    # strict: the lower box index keeps a tie
        best[win] = u[win]
        out["arg"][win] = j
    for j in range(n):
        held = out["arg"] == j
        if held.any():
            out["tmax"][j], out["umax"][j] = out["t"][j, held].max(), out["u"][j, held].max()
            out["quality"][held] = out["t"][j, held] / (out["tmax"][j] + TAL_EPS) * out["umax"][j]
    return out


def tal_targets_bbox(image_shape, annotations: np.ndarray, cls_logits: np.ndarray, reg: np.ndarray, mask_shape=None,
                     topk: int = TAL_TOPK, shapes_callback=None, anchors: Optional[np.ndarray] = None):
    """Task-aligned targets for one image, the float64 oracle: ``(labels (A, C) with -1 rows for ignore, regression
    (A, 4), state (A,), quality (A,))``.  Positives get state 1, the box's label and the usual regression target;
    everything else state 0, label 0 and a zero regression target -- there is no ignore band -- except that anchors
    centred outside the image are ignored last, positives included (their quality is 0 like every non-positive row's)."""
    if anchors is None:
        anchors = anchors_for_shape(image_shape, shapes_callback=shapes_callback)
    anchors = np.asarray(anchors, dtype=np.float64)
    A = anchors.shape[0]
    num_classes = np.asarray(cls_logits).shape[-1]
    annotations = np.asarray(annotations, dtype=np.float64).reshape(-1, 5)
    r = tal_assign(anchors, level_table(image_shape, shapes_callback), annotations, cls_logits, reg, topk)
    pos = r["arg"] >= 0
    labels = np.zeros((A, num_classes))
    state = np.zeros((A,))
    regression = np.zeros((A, 4))
    if pos.any():
        matched = annotations[r["arg"][pos]]
        labels[np.nonzero(pos)[0], matched[:, 4].astype(int)] = 1
        state[pos] = 1
        regression[pos] = bbox_transform(anchors[pos], matched[:, :4])
    mh, mw = (image_shape if mask_shape is None else mask_shape)[:2]
    cx = (anchors[:, 0] + anchors[:, 2]) / 2
    cy = (anchors[:, 1] + anchors[:, 3]) / 2
    outside = (cx >= mw) | (cy >= mh)
    labels[outside, :] = -1
    state[outside] = -1
    return labels, regression, state, np.where(state == 1, r["quality"], 0.0)


def tal_targets_torch(anchors: torch.Tensor, levels, gt: torch.Tensor, gt_count: torch.Tensor, mask_hw: torch.Tensor,
                      cls_logits: torch.Tensor, reg: torch.Tensor, topk: int = TAL_TOPK,
                      centers: Optional[torch.Tensor] = None):
    """Batched fp32 task-aligned targets: the arithmetic of
    ``tal_assign`` in fp32 torch ops, one image at a time ((G, A) intermediates).  ``cls_logits`` (B, A, C) and ``reg``
    (B, A, 4) are the model's detached outputs in any float dtype.  Returns ``(state (B, A) int8, label (B, A) int32,
    regression (B, A, 4) f32, quality (B, A) f32)``; nothing depends on the data in shape or control flow."""
    topk = _check_topk(topk)
    B, G = gt.shape[0], gt.shape[1]
    A = anchors.shape[0]
    dev = anchors.device
    lv, A0 = _check_levels(levels, A)
    f32 = torch.float32
    C = cls_logits.shape[-1]
    if cls_logits.shape[:2] != (B, A) or reg.shape != (B, A, 4):
        raise ValueError("tal_targets_torch: logits (B, A, C) and deltas (B, A, 4) for {} images of {} anchors expected, "
                         "got {} and {}".format(B, A, tuple(cls_logits.shape), tuple(reg.shape)))
    gt = gt.to(f32)
    cnt = gt_count.to(dev).to(torch.int64)
    cc = _tal_centres(lv, A0)
    ccx, ccy = torch.from_numpy(cc[0]).to(dev, f32), torch.from_numpy(cc[1]).to(dev, f32)
    a1, b1, a2, b2 = anchors.to(f32).unbind(-1)
    aw, ah = a2 - a1, b2 - b1
    zero = torch.zeros((), dtype=f32, device=dev)
    k = min(topk, A)
    states, labels, regs, quals = [], [], [], []
    for b in range(B if G else 0):
        d = reg[b].detach().to(f32)
        qx1, qy1 = a1 + (d[:, 0] * BOX_STD) * aw, b1 + (d[:, 1] * BOX_STD) * ah
        qx2, qy2 = a2 + (d[:, 2] * BOX_STD) * aw, b2 + (d[:, 3] * BOX_STD) * ah
        px1, px2 = torch.minimum(qx1, qx2), torch.maximum(qx1, qx2)
        py1, py2 = torch.minimum(qy1, qy2), torch.maximum(qy1, qy2)
        valid = (torch.arange(G, device=dev) < cnt[b])[:, None]                      # (G, 1)
        # rows past the count may hold anything: they are replaced before any arithmetic
        box = torch.where(valid, gt[b, :, :4], zero)
        lab = torch.where(valid[:, 0], gt[b, :, 4], zero).to(torch.int64).clamp(0, C - 1)
        x1, y1, x2, y2 = [box[:, i, None] for i in range(4)]
        iw = (torch.minimum(px2, x2) - torch.maximum(px1, x1)).clamp_min(0)
        ih = (torch.minimum(py2, y2) - torch.maximum(py1, y1)).clamp_min(0)
        inter = iw * ih
        u = inter / ((((px2 - px1) * (py2 - py1))[None] + (x2 - x1) * (y2 - y1) - inter) + TAL_EPS)   # (G, A)
        xs = cls_logits[b].detach().to(f32)[:, lab].t()                                                 # (G, A)
        s = 1.0 / (1.0 + torch.exp(-xs))
        u2 = u * u
        t = s * (u2 * u2 * u2)
        inside = torch.minimum(torch.minimum(ccx - x1, ccy - y1), torch.minimum(x2 - ccx, y2 - ccy)) > ATSS_INSIDE_EPS
        cand = inside & (u > 0) & valid
        # (t descending, index ascending): a stable ascending sort of -t, the non-candidates last
        order = torch.sort(torch.where(cand, -t, torch.ones_like(t)), dim=1, stable=True)[1][:, :k]
        sel = torch.zeros_like(cand).scatter_(1, order, True) & cand
        score = torch.where(sel, u, -torch.ones_like(u))
        best = score.max(dim=0)[0]                                                                      # (A,)
        is_pos = best > 0
        gidx = torch.arange(G, device=dev)[:, None].expand(G, A)
        arg = torch.where(sel & (score == best[None]), gidx, torch.full_like(gidx, G)).min(dim=0)[0]
        argc = arg.clamp(max=G - 1)
        held = (gidx == arg[None]) & is_pos[None]
        tmax = torch.where(held, t, zero).max(dim=1)[0]
        umax = torch.where(held, u, zero).max(dim=1)[0]
        ta = t.gather(0, argc[None])[0]
        q = torch.where(is_pos, ta / (tmax[argc] + TAL_EPS) * umax[argc], zero)
        matched = gt[b][argc]
        r = torch.stack([(matched[:, 0] - a1) / aw, (matched[:, 1] - b1) / ah,
                         (matched[:, 2] - a2) / aw, (matched[:, 3] - b2) / ah], -1)
        r = (r - BOX_MEAN) / BOX_STD
        regs.append(torch.where(is_pos[:, None], r, zero))
        labels.append(torch.where(is_pos, matched[:, 4].to(torch.int32), torch.zeros((), dtype=torch.int32, device=dev)))
        states.append(is_pos.to(torch.int8))
        quals.append(q)
    if G:
        state, label, regression, quality = (torch.stack(states), torch.stack(labels), torch.stack(regs),
                                             torch.stack(quals))
    else:
        state = torch.zeros((B, A), dtype=torch.int8, device=dev)
        label = torch.zeros((B, A), dtype=torch.int32, device=dev)
        regression = torch.zeros((B, A, 4), dtype=f32, device=dev)
        quality = torch.zeros((B, A), dtype=f32, device=dev)
    if centers is None:
        centers = torch.from_numpy(centers_round_down(anchors.double().cpu().numpy())).to(dev)
    mh = mask_hw[:, 0].to(dev).to(f32)[:, None]
    mw = mask_hw[:, 1].to(dev).to(f32)[:, None]
    outside = (centers[None, :, 0] >= mw) | (centers[None, :, 1] >= mh)
    state = torch.where(outside, torch.full_like(state, -1), state)
    quality = torch.where(state == 1, quality, zero)
    return state, label, regression, quality
