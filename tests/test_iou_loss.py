"""The IoU regression losses (GIoU, DIoU, CIoU) on the CPU: the torch expression of ``ops/losses.py`` (the CPU path
and the oracle of the HIP kernel) against a closed-form float64 gradient written out by hand and against differences,
its special cases, ``Trainer(regression_loss=...)``, what checkpoints record and the two flags of ``train.py``."""
import json
import math
import os

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.io import checkpoint
from batchai_retinanet_horovod_coco_amd.ops import losses as L

KINDS = ["giou", "diou", "ciou"]
S = 0.2         # BOX_STD
EPS = 1e-7


# ------------------------------------------------------------------------------------------------ inputs
def _decode(an, d):
    aw, ah = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    return (an[:, 0] + S * d[:, 0] * aw, an[:, 1] + S * d[:, 1] * ah, an[:, 2] + S * d[:, 2] * aw,
            an[:, 3] + S * d[:, 3] * ah)


def _selections(an, pred, target):
    """The eight differences a selection of the loss looks at, each relative to the anchor's side (numpy, (N, 8))."""
    aw, ah = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    gx1, gy1, gx2, gy2 = _decode(an, target)
    qx1, qy1, qx2, qy2 = _decode(an, pred)
    px1, px2, py1, py2 = np.minimum(qx1, qx2), np.maximum(qx1, qx2), np.minimum(qy1, qy2), np.maximum(qy1, qy2)
    iwr = np.minimum(px2, gx2) - np.maximum(px1, gx1)
    ihr = np.minimum(py2, gy2) - np.maximum(py1, gy1)
    return np.stack([(qx1 - qx2) / aw, (qy1 - qy2) / ah, (px1 - gx1) / aw, (px2 - gx2) / aw, (py1 - gy1) / ah,
                     (py2 - gy2) / ah, iwr / aw, ihr / ah], 1)


def _rows(seed, n=400, margin=1e-3):
    """float64 anchors, predicted and target deltas (numpy), every row at least ``margin`` of the anchor's side from
    every tie; overlapping, disjoint and flipped predictions all occur."""
    rng = np.random.RandomState(seed)
    xy = rng.uniform(0, 300, (n, 2))
    wh = rng.uniform(16, 160, (n, 2))
    an = np.concatenate([xy, xy + wh], 1)
    target = rng.randn(n, 4) * 0.6
    pred = target + rng.randn(n, 4) * np.where(rng.rand(n, 1) < 0.5, 1.0, 6.0)
    sel = _selections(an, pred, target)
    keep = (np.abs(sel) >= margin).all(1)
    an, pred, target, sel = an[keep], pred[keep], target[keep], sel[keep]
    flipped = (sel[:, 0] > 0) | (sel[:, 1] > 0)
    disjoint = (sel[:, 6] < 0) | (sel[:, 7] < 0)
    few = n // 20
    assert keep.sum() > 0.9 * n and flipped.sum() >= few and disjoint.sum() >= few and (~disjoint & ~flipped).sum() >= few
    return an, pred, target


def _t(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


# ------------------------------------------------------------------------------------------------ closed form (GIoU)
def _giou_by_hand(an, pred, target):
    """GIoU per row and d GIoU / d pred, every derivative written out (numpy float64, away from ties)."""
    aw, ah = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    gx1, gy1, gx2, gy2 = _decode(an, target)
    qx1, qy1, qx2, qy2 = _decode(an, pred)
    fx, fy = qx1 > qx2, qy1 > qy2
    px1, px2 = np.where(fx, qx2, qx1), np.where(fx, qx1, qx2)
    py1, py2 = np.where(fy, qy2, qy1), np.where(fy, qy1, qy2)
    pw, ph = px2 - px1, py2 - py1
    iwr, ihr = np.minimum(px2, gx2) - np.maximum(px1, gx1), np.minimum(py2, gy2) - np.maximum(py1, gy1)
    iw, ih = np.maximum(iwr, 0), np.maximum(ihr, 0)
    inter = iw * ih
    union = pw * ph + (gx2 - gx1) * (gy2 - gy1) - inter + EPS
    cw, ch = np.maximum(px2, gx2) - np.minimum(px1, gx1), np.maximum(py2, gy2) - np.minimum(py1, gy1)
    c = cw * ch + EPS
    loss = 1 - inter / union + (c - union) / c
    # derivatives with respect to the ordered corners (px1, px2, py1, py2)
    d_inter = [np.where((iwr > 0) & (px1 > gx1), -ih, 0.0), np.where((iwr > 0) & (px2 < gx2), ih, 0.0),
               np.where((ihr > 0) & (py1 > gy1), -iw, 0.0), np.where((ihr > 0) & (py2 < gy2), iw, 0.0)]
    d_area = [-ph, ph, -pw, pw]
    d_c = [np.where(px1 < gx1, -ch, 0.0), np.where(px2 > gx2, ch, 0.0), np.where(py1 < gy1, -cw, 0.0),
           np.where(py2 > gy2, cw, 0.0)]
    g = []
    for di, da, dc in zip(d_inter, d_area, d_c):
        du = da - di
        d_iou = (di * union - inter * du) / union ** 2
        d_ratio = (du * c - union * dc) / c ** 2           # d (U / C); L = 2 - IoU - U / C
        g.append(-d_iou - d_ratio)
    # back through the ordering and the decode
    grad = np.stack([S * aw * np.where(fx, g[1], g[0]), S * ah * np.where(fy, g[3], g[2]),
                     S * aw * np.where(fx, g[0], g[1]), S * ah * np.where(fy, g[2], g[3])], 1)
    return loss, grad


def test_giou_gradient_against_the_closed_form():
    an, pred, target = _rows(0)
    ref_loss, ref_grad = _giou_by_hand(an, pred, target)
    a, p, t = _t(an, pred, target)
    p.requires_grad_(True)
    loss = L.iou_loss_rows(a, p, t, "giou")
    loss.sum().backward()
    assert np.allclose(loss.detach().numpy(), ref_loss, rtol=1e-12, atol=1e-13)
    scale = np.abs(ref_grad).max(1, keepdims=True)
    assert (np.abs(p.grad.numpy() - ref_grad) <= 1e-11 * scale).all()
    assert (scale > 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_gradcheck(kind):
    an, pred, target = _rows(1, n=40)
    a, p, t = _t(an, pred, target)
    alpha = None
    if kind == "ciou":
        # the backward holds alpha fixed: differences must hold it fixed too
        gx1, gy1, gx2, gy2 = _decode(an, target)
        qx1, qy1, qx2, qy2 = _decode(an, pred)
        v = 4 / math.pi ** 2 * (np.arctan((gx2 - gx1) / (gy2 - gy1 + EPS))
                                - np.arctan(np.abs(qx2 - qx1) / (np.abs(qy2 - qy1) + EPS))) ** 2
        both = [L.iou_loss_rows(a, p, t, k).numpy() for k in ("ciou", "diou")]
        alpha = torch.from_numpy((both[0] - both[1]) / v)
        assert bool((alpha > 0).all()) and bool((alpha < 1).all())
    p.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: L.iou_loss_rows(a, x, t, kind, alpha=alpha), (p,), eps=1e-6, atol=1e-7,
                                    rtol=1e-5)


# ------------------------------------------------------------------------------------------------ special cases
def _one(an, pred, target, kind):
    a, p, t = (torch.tensor([v], dtype=torch.float64) for v in (an, pred, target))
    return L.iou_loss_rows(a, p, t, kind).item()


@pytest.mark.parametrize("kind", KINDS)
def test_special_cases(kind):
    an = [10.0, 20.0, 74.0, 52.0]
    t = [0.3, -0.2, 0.5, 0.7]
    assert abs(_one(an, t, t, kind)) < 1e-9                       # the prediction is the target
    far = [40.0, 40.0, 41.0, 41.0]                                # 8 anchor sides away: disjoint
    assert _one(an, far, t, kind) > 1.0
    if kind == "giou":
        assert _one(an, far, t, kind) < 2.0
    # a flipped prediction and its ordered twin: corners (x1, x2) exchanged through the deltas
    aw = an[2] - an[0]
    p = [0.4, 0.1, -0.6, 0.9]
    qx1, qx2 = an[0] + S * p[0] * aw, an[2] + S * p[2] * aw
    flipped = [(qx2 - an[0]) / (S * aw), p[1], (qx1 - an[2]) / (S * aw), p[3]]
    assert flipped[0] > 0 and an[0] + S * flipped[0] * aw > an[2] + S * flipped[2] * aw
    assert abs(_one(an, p, t, kind) - _one(an, flipped, t, kind)) < 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_only_positive_rows_count(kind):
    an, pred, target = _rows(2, n=60)
    n = an.shape[0] // 3 * 3
    a, p, t = _t(an[:n // 3], pred[:n].reshape(3, -1, 4), target[:n].reshape(3, -1, 4))
    a = a.float()
    state = torch.from_numpy(np.random.RandomState(3).randint(-1, 2, (3, n // 3))).to(torch.int8)
    p = p.float().requires_grad_(True)
    loss = L.iou_loss(p, t.float(), state, a, kind, weight=2.0, backend="torch")
    loss.backward()
    pos = state == 1
    rows = L.iou_loss_rows(a[None].expand(3, -1, 4)[pos], p.detach()[pos], t.float()[pos], kind)
    assert torch.allclose(loss, 2.0 * rows.sum() / pos.sum(), rtol=1e-6)
    assert not p.grad[~pos].any() and bool(p.grad[pos].abs().sum(1).gt(0).all())
    # garbage in rows that do not count changes nothing
    p2 = p.detach().clone()
    p2[~pos] = float("nan")
    assert torch.equal(L.iou_loss(p2, t.float(), state, a, kind, weight=2.0, backend="torch"), loss.detach())
    # no positives: 0, not 0 / 0
    none = L.iou_loss(p.detach(), t.float(), torch.zeros_like(state), a, kind, backend="torch")
    assert none.item() == 0.0
    with pytest.raises(ValueError):
        L.iou_loss(p, t.float(), state, a, "iou", backend="torch")


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(seed=0, **kw):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    torch.manual_seed(seed)
    model = models.backbone("resnet18").retinanet(3)
    return Trainer(model, lr=1e-3, clipnorm=0.0, device=torch.device("cpu"), **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_trainer_trains(kind):
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    tr = _trainer(regression_loss=kind, regression_weight=2.0)
    b = make_batch(1, 64, 96, num_classes=3, max_boxes=3, generator=torch.Generator().manual_seed(5))
    w0 = tr.flat.data.clone()
    for _ in range(3):
        logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
        assert all(math.isfinite(float(v)) for v in logs.values())
    assert float(logs["regression_loss"]) > 0 and not torch.equal(w0, tr.flat.data)
    reg, _ = tr.forward_losses(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    assert math.isfinite(float(reg)) and float(reg) > 0


def test_trainer_argument_checks():
    with pytest.raises(ValueError, match="regression_weight"):
        _trainer(regression_weight=2.0)
    with pytest.raises(ValueError, match="regression_weight"):
        _trainer(regression_loss="smooth_l1", regression_weight=0.5)
    with pytest.raises(ValueError, match="regression_loss"):
        _trainer(regression_loss="iou")
    assert _trainer(regression_loss="smooth_l1").regression_loss == "smooth_l1"


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_checkpoint_records_the_loss(tmp_path, ext):
    for kind, weight in (("giou", 1.0), ("diou", 2.5), ("ciou", 1.0)):
        tr = _trainer(regression_loss=kind, regression_weight=weight)
        cfg = checkpoint.training_config(tr.base_optimizer)
        assert cfg["loss"] == {"regression": "_" + kind, "classification": "_focal"}
        assert cfg.get("regression_weight") == (weight if weight != 1.0 else None)
        path = str(tmp_path / "{}.{}".format(kind, ext))
        checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
        assert checkpoint.stored_regression_loss(path) == kind
        assert checkpoint.stored_regression_weight(path) == weight
        assert checkpoint.stored_optimizer_class(path) == "Adam"
    plain = _trainer()
    path = str(tmp_path / ("plain." + ext))
    checkpoint.save_checkpoint(path, plain.model, plain.base_optimizer, epoch=1)
    assert checkpoint.stored_regression_loss(path) == "smooth_l1" and checkpoint.stored_regression_weight(path) == 1.0
    weights_only = str(tmp_path / ("weights." + ext))
    checkpoint.save_checkpoint(weights_only, plain.model, None)
    assert checkpoint.stored_regression_loss(weights_only) is None


def test_default_training_config_is_unchanged():
    """Without the new arguments the stored training_config is, byte for byte, the one written before they existed."""
    for tr in (_trainer(), _trainer(regression_loss="smooth_l1")):
        opt = tr.base_optimizer
        before = json.dumps({"optimizer_config": {"class_name": "Adam", "config": opt.get_config()},
                             "loss": {"regression": "_smooth_l1", "classification": "_focal"},
                             "metrics": [], "sample_weight_mode": None, "loss_weights": None})
        assert json.dumps(checkpoint.training_config(opt)) == before
        assert not hasattr(opt, "regression_loss")


# ------------------------------------------------------------------------------------------------ CLI
def test_flags_parse():
    a = T.parse_args(["coco", "/x"])
    assert a.regression_loss == "smooth_l1" and a.regression_weight == 1.0
    a = T.parse_args(["--regression-loss", "ciou", "--regression-weight", "2.5", "coco", "/x"])
    assert (a.regression_loss, a.regression_weight) == ("ciou", 2.5)
    assert T.build_parser().get_default("regression_loss") is None
    with pytest.raises(SystemExit):
        T.parse_args(["--regression-loss", "iou", "coco", "/x"])
    with pytest.raises(SystemExit, match="regression-weight"):
        T.parse_args(["--regression-weight", "2", "coco", "/x"])
    with pytest.raises(SystemExit, match="regression-weight"):
        T.parse_args(["--regression-loss", "giou", "--regression-weight", "0", "coco", "/x"])
    assert "giou" in T.build_parser().format_help()


def test_flags_against_snapshot(tmp_path, recwarn):
    tr = _trainer(regression_loss="diou", regression_weight=2.0)
    path = str(tmp_path / "diou.h5")
    checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
    a = T.parse_args(["--snapshot", path, "coco", "/x"])                     # the file decides
    assert (a.regression_loss, a.regression_weight) == ("diou", 2.0)
    a = T.parse_args(["--snapshot", path, "--regression-loss", "diou", "--regression-weight", "3", "coco", "/x"])
    assert (a.regression_loss, a.regression_weight) == ("diou", 3.0)
    assert not [w for w in recwarn.list if "regression-loss" in str(w.message)]
    with pytest.warns(UserWarning, match="regression-loss giou differs.*diou"):   # the flag wins
        a = T.parse_args(["--snapshot", path, "--regression-loss", "giou", "coco", "/x"])
    assert (a.regression_loss, a.regression_weight) == ("giou", 1.0)
    with pytest.warns(UserWarning, match="regression-loss smooth_l1 differs"):
        a = T.parse_args(["--snapshot", path, "--regression-loss", "smooth_l1", "coco", "/x"])
    assert (a.regression_loss, a.regression_weight) == ("smooth_l1", 1.0)


def test_cli_trains_snapshots_and_resumes(tmp_path):
    common = ["--no-weights", "--backbone", "resnet18", "--batch-size", "2", "--image-min-side", "64",
              "--image-max-side", "96", "--snapshot-path", str(tmp_path / "snap"), "--tensorboard-dir", "",
              "--device", "cpu", "--workers", "1", "--seed", "1", "--no-evaluation", "--lr", "1e-4"]
    data = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "4", "--max-boxes", "3"]
    h = T.main(common + ["--regression-loss", "giou", "--regression-weight", "2", "--epochs", "1", "--steps", "2"] + data)
    assert len(h.history["loss"]) == 1 and all(math.isfinite(v) for v in h.history["regression_loss"])
    ck = str(tmp_path / "snap" / "checkpoint-01.h5")
    assert os.path.exists(ck) and checkpoint.stored_regression_loss(ck) == "giou"
    assert checkpoint.stored_regression_weight(ck) == 2.0
    # resume without the flags: the snapshot says giou x 2, and the next snapshot says so again
    h2 = T.main(["--snapshot", ck] + common[1:] + ["--epochs", "2", "--steps", "1"] + data)
    assert h2.epoch == [1]
    ck2 = str(tmp_path / "snap" / "checkpoint-02.h5")
    assert checkpoint.stored_regression_loss(ck2) == "giou" and checkpoint.stored_regression_weight(ck2) == 2.0
