"""ops/boxes.py soft_nms, filter_detections(nms_kind=...), the CLI flags, and the margin of the GPU cases' inputs."""
import math

import pytest
import torch

import soft_nms_common as S
from batchai_retinanet_horovod_coco_amd.bin import train as cli
from batchai_retinanet_horovod_coco_amd.ops import boxes as box_ops

KINDS = ("linear", "gaussian")


def _scalar_soft_nms(boxes, scores, kind, thr, sigma, floor, D):
    """The rule of ``box_ops.soft_nms``'s docstring, one double at a time."""
    def iou(a, b):
        inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
        union = sum(max(r[2] - r[0], 0.0) * max(r[3] - r[1], 0.0) for r in (a, b)) - inter
        return inter / union if union > 0 else 0.0
    s, live, out = list(scores), [True] * len(scores), []
    while len(out) < D and any(live):
        i = max((j for j in range(len(s)) if live[j]), key=lambda j: (s[j], -j))
        if s[i] <= floor:
            break
        out.append((i, s[i]))
        live[i] = False
        for j in range(len(s)):
            if live[j]:
                u = iou(boxes[i], boxes[j])
                s[j] *= (1 - u if u > thr else 1.0) if kind == "linear" else math.exp(-(u * u) / sigma)
                live[j] = s[j] > floor
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_soft_nms_matches_scalar_loop(kind):
    g = torch.Generator().manual_seed(1)
    xy = torch.rand(12, 2, generator=g, dtype=torch.float64) * 40
    boxes = torch.cat([xy, xy + 20 + torch.rand(12, 2, generator=g, dtype=torch.float64) * 30], 1)
    scores = torch.rand(12, generator=g, dtype=torch.float64) * 0.9 + 0.1
    scores[5] = scores[2]                                   # an exact tie: the lower index first
    idx, dec = box_ops.soft_nms(boxes, scores, kind, 0.3, 0.5, 0.15, 8)
    ref = _scalar_soft_nms(boxes.tolist(), scores.tolist(), kind, 0.3, 0.5, 0.15, 8)
    assert 2 <= len(ref) and idx.tolist() == [i for i, _ in ref] and dec.dtype == torch.float64
    assert torch.allclose(dec, torch.tensor([v for _, v in ref], dtype=torch.float64), rtol=1e-14, atol=0)


def test_soft_nms_identical_boxes():
    boxes = torch.tensor([[0.0, 0.0, 10.0, 10.0]] * 3, dtype=torch.float64)
    scores = torch.tensor([0.9, 0.8, 0.7], dtype=torch.float64)
    idx, dec = box_ops.soft_nms(boxes, scores, "linear", 0.5, 0.5, 0.05, 10)
    assert idx.tolist() == [0] and dec.tolist() == [0.9]                  # IoU 1: weight 0
    idx, dec = box_ops.soft_nms(boxes, scores, "gaussian", 0.5, 0.5, 0.001, 10)
    want = [0.9, 0.8 * math.exp(-2.0), 0.7 * math.exp(-4.0)]               # exp(-1 / sigma), exp(-2 / sigma)
    assert idx.tolist() == [0, 1, 2] and dec.tolist() == pytest.approx(want, rel=1e-14)
    idx, dec = box_ops.soft_nms(boxes, scores, "gaussian", 0.5, 0.5, 0.05, 10)
    assert idx.tolist() == [0, 1]                                          # 0.7 * exp(-4) = 0.0128 <= min_score
    for bad in (dict(sigma=0.0), dict(min_score=-0.1), dict(kind="hard")):
        with pytest.raises(ValueError):
            box_ops.soft_nms(boxes, scores, **dict(dict(kind="gaussian", sigma=0.5, min_score=0.05), **bad))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("class_specific", [True, False])
def test_filter_detections_soft_kinds(kind, class_specific):
    anchors, deltas, logits = S.inputs("odd_fp32", kind)
    boxes = box_ops.clip_boxes(box_ops.bbox_transform_inv(anchors[None], deltas), 300.0, 300.0)[0]
    b, s, l = box_ops.filter_detections(boxes[:300], torch.sigmoid(logits[0, :300]), max_detections=400, nms_kind=kind,
                                        class_specific_filter=class_specific, backend="torch")
    n = int((s >= 0).sum())
    assert b.shape == (400, 4) and s.shape == (400,) and l.shape == (400,) and l.dtype == torch.int32 and 0 < n < 400
    assert bool((s[:n] > 0.05).all()) and bool((s[:n - 1] >= s[1:n]).all()) and bool((l[:n] >= 0).all())
    assert bool((s[n:] == -1).all()) and bool((l[n:] == -1).all()) and bool((b[n:] == -1).all())


@pytest.mark.parametrize("argv", [["--soft-nms-sigma", "0.3"], ["--soft-nms-min-score", "0.01"],
                                  ["--nms", "soft-gaussian", "--soft-nms-sigma", "0"],
                                  ["--nms", "soft-linear", "--soft-nms-min-score", "-1"]])
def test_cli_flags(argv):
    with pytest.raises(SystemExit):
        cli.parse_args(argv + ["synthetic"])
    args = cli.parse_args(["--nms", "soft-gaussian", "--nms-threshold", "0.4", "--soft-nms-sigma", "0.3", "synthetic"])
    assert cli.nms_kwargs(cli.parse_args(["synthetic"])) == {} and cli.nms_kwargs(args) == dict(
        nms_threshold=0.4, nms_kind="gaussian", soft_nms_sigma=0.3, soft_nms_min_score=None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,D", [("crowded", 100), ("crowded", 10), ("odd_fp32", 50), ("slots", 100)])
def test_input_margin(case, D, kind):
    """An assertion on the GPU cases' inputs: the fp32 torch form takes the float64 reference's decisions, and the
    reference's decision margin is at least ten times the fp32 form's worst score deviation e."""
    e, margin = S.allowance(case, kind, D), S.run(case, kind, D)[1]
    print("\n%s %s D=%d: e = %.3e, margin = %.3e (%.0f e)" % (case, kind, D, e, margin, margin / e))
    assert margin >= 10 * e
