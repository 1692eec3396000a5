"""Helpers of test_tal.py: test_atss_gpu.py's geometry and boxes, the predictions, the float64 oracle per image, the
fp32 torch form's expressions emulated in numpy, and which anchors a comparison must excuse.

Geometry: the 15,354 anchors of a 256 x 320 padded image (the last block of 256 is partial), levels 32x40, 16x20, 8x10,
4x5 and 2x3, 12 / 300 boxes (one and two LDS tiles) with per-image counts [G, 0, G // 2], 80 classes.

What is excused.  With ``t_k`` the metric of a box's last selected candidate and ``t_k1`` that of its first candidate
not selected (float64, the oracle's order), an fp32 computation whose metrics are off by a relative ``eps`` can only
decide differently about a selected candidate with ``t <= t_k1 (1 + eps)`` or an unselected one with
``t >= t_k (1 - eps)``; and between two boxes that both selected an anchor, only when the two largest ``u`` lie within
``eps`` of each other without being equal (equal ones, a duplicated box, go to the lower index in any precision)."""
import numpy as np
import torch

from batchai_retinanet_horovod_coco_amd.ops import anchors as A

PAD_HW = (256, 320)
NUM_CLASSES = 80
HWS = [PAD_HW, (200, 300), (200, 300)]
COUNTS = lambda G: [G, 0, G // 2]                                       # noqa: E731
# index of each special box within an image's rows (all below 6 = 12 // 2)
ANCHOR_BOX, CORNER, BOUNDARY, TINY, DUP = 0, 1, 2, 3, 4

_CACHE = {}


def anchors():
    """(fp32 anchors, the same in float64, centres rounded down to fp32, level table) -- computed once."""
    if "a" not in _CACHE:
        a32 = A.anchors_for_shape(PAD_HW).astype(np.float32)
        a64 = a32.astype(np.float64)
        lv = A.level_table(PAD_HW)
        assert a32.shape[0] == 15354 and a32.shape[0] % 256 == 250
        assert lv[:, 1:3].tolist() == [[32, 40], [16, 20], [8, 10], [4, 5], [2, 3]]
        _CACHE["a"] = (a32, a64, A.centers_round_down(a64), lv)
    return _CACHE["a"]


def _boxes(rng, n, hw):
    """n boxes [x1, y1, x2, y2, label] with integer corners inside an image of (H, W) = hw (test_targets_gpu.py's)."""
    H, W = hw
    w = rng.randint(6, 160, size=n)
    h = rng.randint(6, 160, size=n)
    x1 = (rng.rand(n) * (W - 1 - np.minimum(w, W - 2))).astype(np.int64)
    y1 = (rng.rand(n) * (H - 1 - np.minimum(h, H - 2))).astype(np.int64)
    x2 = np.minimum(x1 + w, W - 1)
    y2 = np.minimum(y1 + h, H - 1)
    return np.stack([x1, y1, x2, y2, rng.randint(0, NUM_CLASSES, size=n)], axis=1).astype(np.float64)


def batch(seed, G):
    """(B, G, 5) boxes as test_atss_gpu.py builds them: the rows from counts[b] on are large valid-looking boxes that
    must not be read; images 0 and 2 hold a box equal to a rounded anchor, a box in the last corner of the padded
    area, one centred on a cell boundary, one too small for any grid centre, a box covering the whole image in the row
    before the last, and in the last row a duplicate of box DUP under another label."""
    rng = np.random.RandomState(seed)
    counts = COUNTS(G)
    _, a64, _, _ = anchors()
    gt = np.zeros((len(counts), G, 5))
    inside = np.nonzero((a64[:, 0] >= 0) & (a64[:, 1] >= 0) & (a64[:, 2] <= 299) & (a64[:, 3] <= 199))[0]
    for b, (c, hw) in enumerate(zip(counts, HWS)):
        gt[b, :c] = _boxes(rng, c, hw)
        gt[b, c:] = [0, 0, hw[1] - 1, hw[0] - 1, NUM_CLASSES - 1]
        gt[b, c::2] = [16, 16, 150, 120, 3]
        if c:
            gt[b, ANCHOR_BOX, :4] = np.round(a64[inside[len(inside) // 2 + b]])
            gt[b, CORNER, :4] = [283, 227, 319, 255]
            gt[b, BOUNDARY, :4] = [50, 40, 110, 120]
            gt[b, TINY, :4] = [101, 101, 103, 103]                # grid centres are at 4 + 8 i: none inside
            gt[b, c - 2, :4] = [0, 0, hw[1] - 1, hw[0] - 1]
            gt[b, c - 1, :4] = gt[b, DUP, :4]
            gt[b, c - 1, 4] = (gt[b, DUP, 4] + 7) % NUM_CLASSES
    assert gt.astype(np.float32).astype(np.float64).tolist() == gt.tolist()       # exact in fp32
    return gt, counts


def predictions(seed, B, kind="trained", dtype=torch.bfloat16):
    """(logits (B, A, C), deltas (B, A, 4)) in ``dtype``.  "trained": logits N(-4, 2), deltas N(0, 1).  "untrained":
    all-zero logits and deltas N(0, 0.05) -- t is u^6 / 2 alone."""
    An = anchors()[0].shape[0]
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "trained":
        logits = torch.randn(B, An, NUM_CLASSES, generator=g) * 2 - 4
        deltas = torch.randn(B, An, 4, generator=g)
    else:
        logits = torch.zeros(B, An, NUM_CLASSES)
        deltas = torch.randn(B, An, 4, generator=g) * 0.05
    return logits.to(dtype), deltas.to(dtype)


def oracle(gt, counts, hws, logits, deltas, topk):
    """Per image: tal_assign's dict plus the oracle's (onehot, reg, state, quality), on the fp32 / bf16 values."""
    _, a64, _, lv = anchors()
    x, d = logits.double().numpy(), deltas.double().numpy()
    out = []
    for b in range(gt.shape[0]):
        ann = gt[b, :counts[b]]
        r = A.tal_assign(a64, lv, ann, x[b], d[b], topk) if counts[b] else {}
        r["onehot"], r["reg"], r["state"], r["q"] = A.tal_targets_bbox(PAD_HW, ann, x[b], d[b], mask_shape=hws[b],
                                                                       topk=topk, anchors=a64)
        out.append(r)
    return out


def excused(r, eps):
    """(near, tie) per anchor, see the module's docstring."""
    t, u, cand, sel = r["t"], r["u"], r["candidate"], r["selected"]
    with np.errstate(invalid="ignore"):
        tk, tk1 = r["cutoff"][:, 0:1], r["cutoff"][:, 1:2]
        near = (sel & (t <= tk1 * (1 + eps))) | (cand & ~sel & (t >= tk * (1 - eps)))     # nan: no such key, False
    us = np.where(sel, u, -1.0)
    if us.shape[0] >= 2:
        part = np.partition(us, -2, axis=0)
        top1, top2 = part[-1], part[-2]
    else:
        top1, top2 = us[0], np.full(us.shape[1], -1.0)
    tie = (top2 > 0) & (top1 - top2 <= eps * top1) & (top1 != top2)
    return near.any(axis=0), tie


def emulate32(boxes, logits, deltas):
    """The fp32 expressions of ``tal_targets_torch`` in numpy float32, every operation rounded on its own, for one
    image: (u, t) (n, A)."""
    a32, _, _, _ = anchors()
    f = np.float32
    d = deltas.float().numpy()
    x = logits.float().numpy()
    assert d.dtype == np.float32 and x.dtype == np.float32
    aw, ah = a32[:, 2] - a32[:, 0], a32[:, 3] - a32[:, 1]
    qx1, qy1 = a32[:, 0] + (d[:, 0] * f(0.2)) * aw, a32[:, 1] + (d[:, 1] * f(0.2)) * ah
    qx2, qy2 = a32[:, 2] + (d[:, 2] * f(0.2)) * aw, a32[:, 3] + (d[:, 3] * f(0.2)) * ah
    px1, px2, py1, py2 = np.minimum(qx1, qx2), np.maximum(qx1, qx2), np.minimum(qy1, qy2), np.maximum(qy1, qy2)
    g = boxes[:, None, :4].astype(f)
    iw = np.maximum(np.minimum(px2, g[..., 2]) - np.maximum(px1, g[..., 0]), f(0))
    ih = np.maximum(np.minimum(py2, g[..., 3]) - np.maximum(py1, g[..., 1]), f(0))
    inter = iw * ih
    uni = ((((px2 - px1) * (py2 - py1))[None] + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])) - inter) + f(1e-7)
    u = inter / uni
    s = f(1) / (f(1) + np.exp(-x[:, boxes[:, 4].astype(np.int64)].T))
    u2 = u * u
    t = s * ((u2 * u2) * u2)
    assert u.dtype == np.float32 and t.dtype == np.float32
    return u, t


def emulated_deviation(gt, counts, refs, logits, deltas):
    """(the largest relative |fp32 - float64| of t over the candidates whose t is at least half their box's cut-off,
    the largest |fp32 - float64| of a quality on the oracle's assignment), the fp32 side emulated on the CPU."""
    f = np.float32
    d_t = d_q = 0.0
    for b, r in enumerate(refs):
        if not counts[b]:
            continue
        u32, t32 = emulate32(gt[b, :counts[b]], logits[b], deltas[b])
        with np.errstate(invalid="ignore", divide="ignore"):
            m = r["candidate"] & (r["t"] >= 0.5 * r["cutoff"][:, 0:1]) & (r["t"] > 0)
            d_t = max(d_t, float((np.abs(t32.astype(np.float64) - r["t"])[m] / r["t"][m]).max()))
        q32 = np.zeros(r["arg"].shape[0], dtype=f)
        for j in np.unique(r["arg"][r["arg"] >= 0]):
            held = r["arg"] == j
            q32[held] = t32[j, held] / (t32[j, held].max() + f(1e-7)) * u32[j, held].max()
        d_q = max(d_q, float(np.abs(q32.astype(np.float64) - r["quality"]).max()))
    return d_t, d_q
