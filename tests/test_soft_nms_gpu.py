"""csrc/kernels/soft_nms.hip through ``native.filter_detections_batched(nms_kind=...)`` against the float64 reference of
soft_nms_common.py, per image as sorted sets.  Boxes get filter.hip's allowance; scores get 4 e, e the fp32 torch form's
worst deviation on the same input (the kernel shares its operation order and differs in expf / sigmoid rounding);
test_soft_nms.py asserts that the reference's decision margin is at least 10 e, so no decision may differ."""
import pytest
import torch

import soft_nms_common as S
from batchai_retinanet_horovod_coco_amd.ops import native as N

pytestmark = pytest.mark.gpu
KINDS = ("linear", "gaussian")


def _run(cuda, case, kind, D, **kw):
    anchors, deltas, logits = (t.to(cuda) for t in S.inputs(case, kind))
    H, W = S.CASES[case][3:5]
    return N.filter_detections_batched(anchors, deltas, logits, H, W, S.THR, S.NMS_THR, D, nms_kind=kind,
                                       soft_nms_sigma=S.SIGMA, **kw)


def _check(got, case, kind, D):
    ref, margin, cuts = S.run(case, kind, D)
    e, worst = S.allowance(case, kind, D), 0.0
    for b, (r, cut) in enumerate(zip(ref, cuts)):
        keep = got[1][b] >= 0
        assert bool((got[1][b][~keep] == -1).all()) and bool((got[2][b][~keep] == -1).all())
        g = torch.cat([got[2][b][keep, None], got[1][b][keep, None], got[0][b][keep]], 1).double().cpu()
        S.check_tied(g, r.shape[0] - S.trim(r, cut, margin).shape[0], cut, margin)
        g = S.sort_rows(S.trim(g, cut, margin, 1), ((2, False), (1, True), (0, False)))
        r = S.sort_rows(S.trim(r, cut, margin), ((3, False), (2, True), (0, False)))
        assert g.shape[0] == r.shape[0] and torch.equal(g[:, 0], r[:, 0]), (b, g.shape, r.shape)
        worst = max(worst, float((g[:, 1] - r[:, 2]).abs().max()))
        assert torch.allclose(g[:, 2:], r[:, 3:], atol=2e-3, rtol=1e-4), (b, (g[:, 2:] - r[:, 3:]).abs().max())
    print("\n%s %s D=%d: score allowance 4 e = %.3e, observed %.3e; box allowance atol 2e-3 rtol 1e-4; margin %.3e"
          % (case, kind, D, 4 * e, worst, margin))
    assert worst <= 4 * e


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,D", [("crowded", 100), ("crowded", 10), ("odd_fp32", 50), ("slots", 100)])
def test_soft_nms_matches_reference(cuda, case, D, kind):
    """~450 candidates per segment (two register slots), picks that stop before the candidates do, fp32 with padded
    classes, and segments of 255 / 256 / 257 / 1 / 0 candidates."""
    _check(_run(cuda, case, kind, D), case, kind, D)


@pytest.mark.parametrize("kind", KINDS)
def test_soft_nms_workspace_form_and_repeat(cuda, kind):
    """The exact workspace form (cap = 64) and a second call give the first call's bits."""
    first = _run(cuda, "crowded", kind, 100)
    for other in (_run(cuda, "crowded", kind, 100, cap=64), _run(cuda, "crowded", kind, 100)):
        assert all(torch.equal(a, b) for a, b in zip(first, other))


def test_hard_kind_is_the_greedy_path(cuda):
    from test_filter_gpu import _check as check_hard, _oracle
    anchors, deltas, logits = (t.to(cuda) for t in S.inputs("crowded", "linear"))
    got = N.filter_detections_batched(anchors, deltas, logits, 400.0, 600.0, max_detections=100, nms_kind="hard")
    assert all(torch.equal(a, b) for a, b in zip(got, N.filter_detections_batched(anchors, deltas, logits, 400.0, 600.0,
                                                                                  max_detections=100)))
    check_hard(got, _oracle(anchors, deltas, logits, 400.0, 600.0, 100))


def test_soft_nms_refusals(cuda):
    """The entry point returns -1 before any launch (so null pointers do); the wrapper raises."""
    def entry(cap=4096, kind=2, D=100):
        return N.lib().mxr_filter_soft_nms(None, None, cap, 0, 0, 8, None, 1, 0.05, None, None, None, None, None, 1, 64,
                                           8, 64.0, 64.0, 0.2, kind, 0.5, 0.5, 0.05, D, None, None, None, None, None)
    assert [entry(D=513), entry(D=0), entry(cap=8192), entry(kind=0), entry(kind=3)] == [-1] * 5
    with pytest.raises(RuntimeError, match="code -1"):
        _run(cuda, "odd_fp32", "gaussian", 513)
    with pytest.raises(ValueError, match="cap"):
        _run(cuda, "odd_fp32", "gaussian", 50, cap=8192)


def test_prediction_model_soft_kind(cuda, monkeypatch):
    """The model dispatches the batched path (4,608 candidates per class); over 512 detections, the torch form."""
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.models.calibrate import calibrate_from_synthetic
    from batchai_retinanet_horovod_coco_amd.models.retinanet import retinanet_bbox
    torch.manual_seed(0)
    model = models.backbone("resnet18").retinanet(8)
    calibrate_from_synthetic(model, torch.device("cpu"), batch=1, height=128, width=192)
    model = model.to(cuda).eval()
    with torch.no_grad():
        model.classification_submodel.final.bias.add_(2.5)
    calls = []
    real = N.filter_detections_batched
    monkeypatch.setattr(N, "filter_detections_batched", lambda *a, **k: calls.append(k) or real(*a, **k))
    x = torch.randn(2, 128, 192, 3, device=cuda) * 50
    pb, ps, pl = retinanet_bbox(model, max_detections=100, nms_kind="gaussian")(x)
    assert [k["nms_kind"] for k in calls] == ["gaussian"]
    assert pb.shape == (2, 100, 4) and ps.shape == (2, 100) and pl.shape == (2, 100)
    assert bool((ps >= 0).any()) and bool((ps[ps >= 0] > 0.05).all())
    floor = 0.9 * float(ps.max())            # a high floor: the torch form loops over picks, keep them few
    pb, ps, pl = retinanet_bbox(model, max_detections=513, nms_kind="gaussian", soft_nms_min_score=floor)(x[:1])
    assert len(calls) == 1 and pb.shape == (1, 513, 4) and ps.shape == (1, 513) and pl.shape == (1, 513)
    assert bool((ps >= 0).any()) and bool((ps[ps >= 0] > floor).all())
