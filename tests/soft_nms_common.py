"""Helpers of test_soft_nms.py / test_soft_nms_gpu.py: the GPU cases' seeded inputs (built on the CPU, so the CPU test
can vet them), the float64 reference -- ``box_ops.soft_nms`` per (image, class) on boxes decoded and clipped in float64
from the same tensors, then the top ``D`` decayed scores -- and its smallest decision margin: the non-zero gaps between
a picked score and the best other live one, the distance of every score from ``min_score`` when it is compared, for
``linear`` of every live IoU from the threshold, and the gap above the cross-class cut after row ``D``.  Exact ties of
untouched equal scores go to the lower index on every side and do not count; only at the cut, equal scores of different
classes (bf16 logits) come in an order the top-k does not define: rows at that score are compared as a subset."""
import torch

from batchai_retinanet_horovod_coco_amd.ops import boxes as box_ops

THR, NMS_THR, SIGMA = 0.05, 0.5, 0.5
# name -> (B, A, C, H, W, dtype, hot, {kind: seed}); the seeds are vetted by test_soft_nms.py::test_input_margin
CASES = {
    "crowded": (2, 3000, 16, 400.0, 600.0, torch.bfloat16, 0.15, {"linear": 0, "gaussian": 27}),
    "odd_fp32": (1, 1500, 5, 300.0, 300.0, torch.float32, 0.05, {"linear": 0, "gaussian": 0}),
    "slots": (1, 600, 8, 300.0, 300.0, torch.bfloat16, None, {"linear": 0, "gaussian": 1}),
}
SLOT_COUNTS = (255, 256, 257, 1, 0)      # candidates of classes 0..4 of "slots": around one register slot (256)
_CACHE = {}


def inputs(case, kind):
    """(anchors fp32, deltas, logits) on the CPU -- test_filter_gpu.py's distribution from a CPU generator."""
    B, A, C, H, W, dtype, hot, seeds = CASES[case]
    g = torch.Generator().manual_seed(seeds[kind])
    ctr = torch.rand(A, 2, generator=g) * torch.tensor([W, H])
    wh = 16 + torch.rand(A, 2, generator=g) * 200
    anchors = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    deltas = (torch.randn(B, A, 4, generator=g) * 0.5).to(dtype)
    logits = torch.randn(B, A, C, generator=g) - 5.0
    if hot is None:
        warm = torch.rand(B, A, C, generator=g) * 4 - 1
        logits = torch.full((B, A, C), -20.0)
        for c, n in enumerate(SLOT_COUNTS):
            logits[:, :n, c] = warm[:, :n, c]
    else:
        logits = torch.where(torch.rand(B, A, C, generator=g) < hot, logits + 6.0, logits)
    return anchors, deltas, logits.to(dtype)


def _margin(boxes, s0, picks, kind):
    s, m = s0.clone(), (s0 - THR).abs().min()
    for i in picks.tolist():
        others = s.clone()
        others[i] = 0
        gap = s[i] - others.max()
        m = torch.minimum(m, gap) if gap > 0 else m
        u = box_ops.box_iou_plain(boxes[i:i + 1], boxes)[0]
        live = others > 0
        if kind == "linear":
            w = torch.where(u > NMS_THR, 1 - u, torch.ones_like(u))
            m = torch.minimum(m, (u[live] - NMS_THR).abs().min()) if live.any() else m
        else:
            w = torch.exp(-(u * u) / SIGMA)
        d = others * w
        changed = live & (w != 1)
        m = torch.minimum(m, (d[changed] - THR).abs().min()) if changed.any() else m
        s = torch.where(d > THR, d, torch.zeros_like(d))
    return m


def sort_rows(rows, keys):
    # lexicographic; keys are (column, descending) from the least to the most significant
    for col, desc in keys:
        rows = rows[torch.argsort(rows[:, col], descending=desc, stable=True)]
    return rows


def run(case, kind, D, dtype=torch.float64):
    """(per image the top D rows ``[label, anchor, score, x1, y1, x2, y2]`` in ``dtype`` sorted by (label, descending
    score, anchor); the margin, float64 only; per image (the cut score, every emitted row at it), -inf where the cut is
    no tie).  Cached."""
    key = (case, kind, D, dtype)
    if key not in _CACHE:
        anchors, deltas, logits = inputs(case, kind)
        H, W = CASES[case][3:5]
        boxes = box_ops.clip_boxes(box_ops.bbox_transform_inv(anchors.to(dtype)[None], deltas.to(dtype)), H, W)
        probs = torch.sigmoid(logits.to(dtype))
        out, cuts, margin = [], [], torch.tensor(float("inf"), dtype=torch.float64)
        for b in range(logits.shape[0]):
            rows = [torch.zeros(0, 7, dtype=dtype)]
            for c in range(logits.shape[2]):
                idx = torch.nonzero(probs[b, :, c] > THR).flatten()
                k, s = box_ops.soft_nms(boxes[b, idx], probs[b, idx, c], kind, NMS_THR, SIGMA, THR, D)
                rows.append(torch.cat([torch.full_like(s, c)[:, None], idx[k].to(dtype)[:, None], s[:, None],
                                       boxes[b, idx[k]]], 1))
                if dtype == torch.float64 and idx.numel():
                    margin = torch.minimum(margin, _margin(boxes[b, idx], probs[b, idx, c], k, kind))
            rows = torch.cat(rows)
            order = torch.argsort(rows[:, 2], descending=True, stable=True)
            top, cut = rows[order[:D]], float("-inf")
            if order.numel() > D:
                cut = float(rows[order[D], 2])
                above = top[top[:, 2] > cut, 2]
                margin = torch.minimum(margin, above.min() - cut) if above.numel() else margin
                cut = cut if float(top[-1, 2]) == cut else float("-inf")
            out.append(sort_rows(top, ((1, False), (2, True), (0, False))))
            cuts.append((cut, rows[rows[:, 2] == cut]))
        _CACHE[key] = (out, float(margin), cuts)
    return _CACHE[key]


def trim(rows, cut, margin, score_col=2):
    return rows[rows[:, score_col] > cut[0] + margin / 2]


def check_tied(got, n, cut, margin):
    """``got`` rows ``[label, score, box]`` at a tied cut: n of them, each another one of the reference's rows there."""
    at = got[(got[:, 1] - cut[0]).abs() < margin / 2]
    assert at.shape[0] == n
    if n:
        d = (at[:, None, [0, 2, 3, 4, 5]] - cut[1][None][:, :, [0, 3, 4, 5, 6]]).abs().amax(-1).min(1)
        assert bool((d.values <= 2e-3).all()) and d.indices.unique().numel() == n


def allowance(case, kind, D):
    """``e``: the worst score deviation of the fp32 torch form from the float64 reference (same picks required)."""
    ref, margin, cuts = run(case, kind, D)
    e = 0.0
    for r, f, cut in zip(ref, run(case, kind, D, torch.float32)[0], cuts):
        r, f = trim(r, cut, margin), trim(f, cut, margin)
        assert r.shape == f.shape and torch.equal(r[:, :2], f[:, :2].double()), "fp32 form picks differ"
        e = max(e, float((r[:, 2] - f[:, 2].double()).abs().max()) if r.numel() else 0.0)
    return e
