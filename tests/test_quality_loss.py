"""The IoU-aware classification losses (``ops.losses.quality_loss``: Quality Focal Loss, Varifocal Loss) on the CPU:
the torch expression in float64 is the oracle of csrc/kernels/quality_loss.hip, so it is itself checked here -- the
per-element gradient of the specification against its autograd and against central differences, ``quality_targets``
against a brute-force IoU, the fp32 form against float64 -- and the switch through Trainer, checkpoints and the CLI.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.io import checkpoint
from batchai_retinanet_horovod_coco_amd.ops import losses as L
from batchai_retinanet_horovod_coco_amd.ops.anchors import anchor_targets_torch, anchors_for_shape

KINDS = list(L.CLS_KINDS)
ALPHA = 0.75
# what the fp32 torch forms need against float64, measured on the CPU: DQ_TORCH and RTOL_F32_TORCH of
# test_quality_loss_gpu.py (the worst over that file's inputs; its docstring has the figures).  On _inputs here (same
# anchors, boxes and noise, another random stream; seeds 0 and 1, noise 1 and 6, printed by test_fp32_against_float64)
# q needs 1.38e-7 .. 2.72e-7 and the gradient 5.94e-7 .. 6.72e-7 |ref| beside that file's allowance for the label
# elements: inside both
DQ_TORCH = 2.91e-7
RTOL_F32_TORCH = 7.04e-7
ATOL = 1e-13


def test_kinds():
    assert L.CLS_KINDS == ("qfl", "vfl")


# ------------------------------------------------------------------------------------------------ inputs
def _inputs(seed=0, noise=1.0, C=5, dtype=torch.float64):
    """The 2,907 anchors of a 96 x 160 image, two images of 12 boxes: anchors (A, 4), logits (B, A, C), reg / reg_t
    (B, A, 4), state (B, A) int8 with a tenth of the rows set to -1, label (B, A) int32."""
    H, W, B, G = 96, 160, 2, 12
    gen = torch.Generator().manual_seed(seed)
    anchors = torch.from_numpy(anchors_for_shape((H, W, 3)).astype(np.float32))
    wh = 12 + 70 * torch.rand(B, G, 2, generator=gen)
    xy = torch.rand(B, G, 2, generator=gen) * (torch.tensor([W, H], dtype=torch.float32) - wh)
    cls = ((torch.arange(B * G) * 11) % C).reshape(B, G, 1).float()
    state, label, reg_t = anchor_targets_torch(anchors, torch.cat([xy, xy + wh, cls], 2), torch.full((B,), G),
                                               torch.tensor([[H, W]] * B))
    state = state.clone()
    state[torch.rand(state.shape, generator=gen) < 0.1] = -1
    reg = reg_t + noise * torch.randn(reg_t.shape, generator=gen)
    x = 6 * torch.randn(B, anchors.shape[0], C, generator=gen)
    return anchors.to(dtype), x.to(dtype), reg.to(dtype), reg_t.to(dtype), state, label


def _iou_by_hand(an, d, t):
    """Plain python floats: the IoU of the decoded boxes of one row."""
    an, d, t = [float(v) for v in an], [float(v) for v in d], [float(v) for v in t]
    aw, ah = an[2] - an[0], an[3] - an[1]
    g = [an[0] + 0.2 * t[0] * aw, an[1] + 0.2 * t[1] * ah, an[2] + 0.2 * t[2] * aw, an[3] + 0.2 * t[3] * ah]
    q = [an[0] + 0.2 * d[0] * aw, an[1] + 0.2 * d[1] * ah, an[2] + 0.2 * d[2] * aw, an[3] + 0.2 * d[3] * ah]
    p = [min(q[0], q[2]), min(q[1], q[3]), max(q[0], q[2]), max(q[1], q[3])]
    iw = max(0.0, min(p[2], g[2]) - max(p[0], g[0]))
    ih = max(0.0, min(p[3], g[3]) - max(p[1], g[1]))
    inter = iw * ih
    return inter / ((p[2] - p[0]) * (p[3] - p[1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter + 1e-7)


def _spec(x, q, state, label, kind):
    """The issue's per-element loss and gradient in float64, unnormalised; x (B, A, C), q (B, A)."""
    C = x.shape[-1]
    lab = (state == 1)[..., None] & (torch.arange(C)[None, None, :] == label.long()[..., None])
    t = torch.where(lab, q[..., None].expand_as(x), torch.zeros_like(x))
    keep = (state != -1)[..., None].to(x.dtype)
    p, om = torch.sigmoid(x), torch.sigmoid(-x)         # om = 1 - p without the cancellation
    sp = x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))
    neg_l = p * p * sp
    neg_g = 2 * p * p * om * sp + p ** 3
    if kind == "qfl":
        l = (p - t) ** 2 * (sp - t * x)
        g = 2 * (p - t) * p * om * (sp - t * x) + (p - t) ** 3
    else:
        soft = lab & (t > 0)
        l = torch.where(soft, t * (sp - t * x), ALPHA * neg_l)
        g = torch.where(soft, t * (p - t), ALPHA * neg_g)
    return l * keep, g * keep, lab


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("noise", [1.0, 6.0])
@pytest.mark.parametrize("kind", KINDS)
def test_float64_gradient_is_the_specification(kind, noise):
    """autograd of the float64 torch expression == the issue's closed-form gradient == central differences; q is
    held fixed: nothing reaches the regression output."""
    anchors, x, reg, reg_t, state, label = _inputs(0, noise)
    x.requires_grad_(True)
    reg.requires_grad_(True)
    loss = L.quality_loss(x, reg, reg_t, state, label, anchors, kind, backend="torch")
    assert loss.dtype == torch.float64
    loss.backward()
    assert reg.grad is None or not reg.grad.any()
    n = max(1, int((state == 1).sum()))
    q = L.quality_targets(anchors, reg.detach(), reg_t, state)
    assert q.dtype == torch.float64 and not q.requires_grad
    l, g, lab = _spec(x.detach(), q, state, label, kind)
    assert abs(loss.item() - l.sum().item() / n) <= 1e-13 * loss.item()
    err = (x.grad - g / n).abs()
    # p - q cancels in the label elements (terms of order 1): an absolute 4e-16 beside the relative bound
    assert bool((err <= (1e-14 * g.abs() + 4e-16) / n).all()), (err * n - 1e-14 * g.abs()).max().item()
    # central differences on the label elements of the positive rows and on a sample of the others
    idx = torch.cat([lab.reshape(-1).nonzero().flatten()[:60], torch.arange(0, x.numel(), 997)])
    h = 1e-4      # the loss is a sum of ~29,000 elements: its rounding, eps loss / 2h, is what limits the difference
    xf = x.detach().reshape(-1)
    for i in idx.tolist():
        up, dn = xf.clone(), xf.clone()
        up[i] += h
        dn[i] -= h
        fd = (L.quality_loss(up.reshape(x.shape), reg.detach(), reg_t, state, label, anchors, kind, backend="torch")
              - L.quality_loss(dn.reshape(x.shape), reg.detach(), reg_t, state, label, anchors, kind,
                               backend="torch")).item() / (2 * h)
        want = x.grad.reshape(-1)[i].item()
        assert abs(fd - want) <= 1e-6 * abs(want) + 1e-9, (i, fd, want)


def test_quality_targets_by_hand():
    an = torch.tensor([[10.0, 20.0, 50.0, 100.0]], dtype=torch.float64)
    t = torch.tensor([0.3, -0.2, 0.1, 0.4], dtype=torch.float64)
    rows = {"identical": t.clone(),
            "disjoint": torch.tensor([30.0, -0.2, 40.0, 0.4], dtype=torch.float64),      # pushed far to the right
            "flipped": torch.tensor([5.5, -0.2, -4.5, 0.4], dtype=torch.float64),        # x1 > x2 after the decode
            "zero_area": torch.tensor([0.3, -0.2, -4.7, 0.4], dtype=torch.float64),      # x2 == x1
            "overlap": torch.tensor([0.9, 0.3, -0.5, 0.1], dtype=torch.float64)}
    reg = torch.stack(list(rows.values()))[:, None, :]                                   # (5, 1, 4): five "images"
    reg_t = t[None, None, :].expand(5, 1, 4)
    state = torch.ones(5, 1, dtype=torch.int8)
    q = L.quality_targets(an, reg, reg_t, state).reshape(-1)
    want = [_iou_by_hand(an[0], r, t) for r in rows.values()]
    assert torch.allclose(q, torch.tensor(want, dtype=torch.float64), rtol=1e-14, atol=0)
    got = dict(zip(rows, q.tolist()))
    assert 0 < 1 - got["identical"] < 1e-9               # 1 - O(1e-7 / area)
    assert got["disjoint"] == 0.0 and got["zero_area"] == 0.0
    assert 0 < got["flipped"] < 1 and 0 < got["overlap"] < 1
    # a flipped prediction is the ordered box
    unflipped = rows["flipped"].clone()
    aw = 40.0
    x1, x2 = 10 + 0.2 * 5.5 * aw, 50 - 0.2 * 4.5 * aw
    unflipped[0], unflipped[2] = (x2 - 10) / (0.2 * aw), (x1 - 50) / (0.2 * aw)
    assert abs(_iou_by_hand(an[0], unflipped, t) - got["flipped"]) < 1e-12
    # rows that are not positive get 0, and the dtype follows the inputs
    state2 = torch.tensor([[1], [0], [-1], [1], [0]], dtype=torch.int8)
    q2 = L.quality_targets(an, reg, reg_t, state2).reshape(-1)
    assert q2[1] == 0 and q2[2] == 0 and q2[4] == 0 and q2[0] == q[0] and q2[3] == q[3]
    assert L.quality_targets(an.float(), reg.float(), reg_t.float(), state).dtype == torch.float32


@pytest.mark.parametrize("noise", [1.0, 6.0])
@pytest.mark.parametrize("seed", [0, 1])
def test_fp32_against_float64(seed, noise):
    """The fp32 torch forms (the CPU training path) against the float64 oracle, under the bound of
    test_quality_loss_gpu.py with the torch yardsticks themselves (no 8 x margin: this is what they were measured
    on)."""
    anchors, x, reg, reg_t, state, label = _inputs(seed, noise)
    q64 = L.quality_targets(anchors, reg.float().double(), reg_t.float().double(), state)
    q32 = L.quality_targets(anchors.float(), reg.float(), reg_t.float(), state)
    dq = (q32.double() - q64).abs().max().item()
    print("seed {} noise {}: worst |q32 - q64| {:.3e}".format(seed, noise, dq))
    assert q32.dtype == torch.float32 and dq <= DQ_TORCH
    n = max(1, int((state == 1).sum()))
    for kind in KINDS:
        x32 = x.float().requires_grad_(True)
        loss32 = L.quality_loss(x32, reg.float(), reg_t.float(), state, label, anchors.float(), kind, backend="torch")
        assert loss32.dtype == torch.float32
        loss32.backward()
        l, g, lab = _spec(x.float().double(), q64, state, label, kind)
        ref = g / n
        p = torch.sigmoid(x.float().double())
        t = torch.where(lab, q64[..., None].expand_as(p), torch.zeros_like(p))
        if kind == "qfl":
            sp = x.float().double().clamp_min(0) + torch.log1p(torch.exp(-x.float().double().abs()))
            b, d, xx = sp - t * x.float().double(), p - t, x.float().double()
            dg_dq = -2 * p * (1 - p) * b - 2 * d * p * (1 - p) * xx - 3 * d * d
            dg_dp = 2 * (p * (1 - p) + d * (1 - 2 * p)) * b + 3 * d * d
        else:
            dg_dq, dg_dp = p - 2 * t, t
        extra = torch.where(lab, dg_dq.abs() * 8 * DQ_TORCH + dg_dp.abs() * 2.0 ** -23 * p, torch.zeros_like(p)) / n
        err = (x32.grad.double() - ref).abs() - ATOL / n - extra
        need = torch.where(ref != 0, err.clamp_min(0) / ref.abs(), torch.zeros_like(err)).max().item()
        print("seed {} noise {} {}: worst rtol needed {:.3e}".format(seed, noise, kind, need))
        assert need <= RTOL_F32_TORCH
        assert abs(loss32.item() - l.sum().item() / n) <= 1e-6 * l.sum().item() / n


# ------------------------------------------------------------------------------------------------ rules
@pytest.mark.parametrize("kind", KINDS)
def test_ignored_rows_and_empty_batches(kind):
    anchors, x, reg, reg_t, state, label = _inputs(0, 6.0)
    x.requires_grad_(True)
    L.quality_loss(x, reg, reg_t, state, label, anchors, kind, backend="torch").backward()
    assert int((state == -1).sum()) > 100 and not x.grad[state == -1].any() and x.grad[state != -1].all()
    # what the ignored rows hold does not matter
    x2 = x.detach().clone()
    x2[state == -1] = 123.0
    a = L.quality_loss(x.detach(), reg, reg_t, state, label, anchors, kind, backend="torch")
    assert torch.equal(a, L.quality_loss(x2, reg, reg_t, state, label, anchors, kind, backend="torch"))
    for fill in (0, -1):        # no positives / all ignored
        s = torch.full_like(state, fill)
        xg = x.detach().clone().requires_grad_(True)
        loss = L.quality_loss(xg, reg, reg_t, s, label, anchors, kind, backend="torch")
        loss.backward()
        assert math.isfinite(loss.item()) and bool(torch.isfinite(xg.grad).all())
        if fill == -1:
            assert loss.item() == 0.0 and not xg.grad.any()
        else:
            c = 1.0 if kind == "qfl" else ALPHA
            p = torch.sigmoid(x.detach())
            assert abs(loss.item() - (c * p * p * torch.nn.functional.softplus(x.detach())).sum().item()) \
                <= 1e-12 * loss.item()


@pytest.mark.parametrize("kind", KINDS)
def test_non_label_classes_take_the_negative_formula(kind):
    """Every class but the label of a positive row, and a VFL label whose q is exactly 0, cost c p^2 softplus(x) with
    the gradient c (2 p^2 (1 - p) softplus(x) + p^3), c = 1 (QFL) / 0.75 (VFL)."""
    anchors, x, reg, reg_t, state, label = _inputs(1, 6.0)
    x.requires_grad_(True)
    L.quality_loss(x, reg, reg_t, state, label, anchors, kind, backend="torch").backward()
    n = max(1, int((state == 1).sum()))
    q = L.quality_targets(anchors, reg, reg_t, state)
    xd = x.detach()
    _, _, lab = _spec(xd, q, state, label, kind)
    c = 1.0 if kind == "qfl" else ALPHA
    p = torch.sigmoid(xd)
    sp = torch.nn.functional.softplus(xd)
    neg = c * (2 * p * p * (1 - p) * sp + p ** 3) / n
    pos_rows = (state == 1)[..., None].expand_as(lab)
    other = pos_rows & ~lab
    assert int(other.sum()) > 100
    assert torch.allclose(x.grad[other], neg[other], rtol=1e-12, atol=0)
    zero_q = lab & (q == 0)[..., None]
    assert int(zero_q.sum()) >= 50
    # VFL sends a label element with q == 0 down the negative formula; QFL's own expression is that formula at q = 0
    assert torch.allclose(x.grad[zero_q], neg[zero_q], rtol=1e-12, atol=0)
    soft = lab & (q > 0)[..., None]
    assert int(soft.sum()) >= 50 and not torch.allclose(x.grad[soft], neg[soft], rtol=1e-3, atol=0)


def test_unknown_kind():
    anchors, x, reg, reg_t, state, label = _inputs()
    with pytest.raises(ValueError, match="kind"):
        L.quality_loss(x, reg, reg_t, state, label, anchors, "gfl", backend="torch")


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(seed=0, **kw):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    torch.manual_seed(seed)
    model = models.backbone("resnet18").retinanet(3)
    return Trainer(model, lr=1e-3, clipnorm=0.0, device=torch.device("cpu"), **kw)


def _batch():
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    return make_batch(1, 64, 96, num_classes=3, max_boxes=3, generator=torch.Generator().manual_seed(5))


@pytest.mark.parametrize("kind", KINDS)
def test_trainer_step_is_autograd_of_quality_loss(kind):
    b = _batch()
    tr = _trainer(classification_loss=kind)
    assert tr.classification_loss == kind
    # the step's gradient (before the optimizer consumes it) against autograd of the losses on a twin
    tr.model.train()
    tr.optimizer.zero_grad()
    reg_loss, cls_loss = tr.forward_backward(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    got = tr.flat.grad.clone()
    twin = _trainer(classification_loss=kind)
    twin.model.train()
    state, label, reg_t, _ = twin.compute_targets(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    out = twin.model(b["images"].to(twin.compute_dtype))
    anchors = twin.anchors.get((64, 96), twin.device, None)
    want_cls = L.quality_loss(out["classification"], out["regression"], reg_t, state, label, anchors, kind,
                              backend="torch")
    want_reg = L.smooth_l1_loss(out["regression"], reg_t, state, backend="torch")
    twin.optimizer.zero_grad()
    (want_reg + want_cls).backward()
    assert torch.equal(cls_loss, want_cls.detach()) and torch.equal(reg_loss, want_reg.detach())
    assert got.any() and torch.equal(got, twin.flat.grad)
    # and it trains
    w0 = tr.flat.data.clone()
    for _ in range(2):
        logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
        assert all(math.isfinite(float(v)) for v in logs.values())
    assert float(logs["classification_loss"]) > 0 and not torch.equal(w0, tr.flat.data)
    _, cls = tr.forward_losses(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    assert math.isfinite(float(cls)) and float(cls) > 0


def test_naming_focal_changes_nothing():
    b = _batch()
    runs = []
    for kw in ({}, {"classification_loss": "focal"}):
        tr = _trainer(**kw)
        logs = [tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"]) for _ in range(2)]
        runs.append((torch.stack([torch.stack([l["loss"], l["classification_loss"]]) for l in logs]),
                     tr.flat.data.clone()))
        assert tr.classification_loss == "focal" and not hasattr(tr.base_optimizer, "classification_loss")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_trainer_refusals(monkeypatch):
    from batchai_retinanet_horovod_coco_amd.ops import fp8
    with pytest.raises(ValueError, match="classification_loss"):
        _trainer(classification_loss="gfl")
    monkeypatch.setattr(fp8, "enabled", lambda: True)
    with pytest.raises(ValueError, match="fp8"):
        _trainer(classification_loss="qfl")
    monkeypatch.undo()
    # a regression output that is not in the classification output's row order
    tr = _trainer(classification_loss="vfl")
    b = _batch()
    state, label, reg_t, npos = tr.compute_targets(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    out = tr.model(b["images"])
    anchors = tr.anchors.get((64, 96), tr.device, None)
    bad = {"classification": out["classification"], "regression": out["regression"][:, :-9]}
    with pytest.raises(ValueError, match="row order"):
        tr._classification_torch(bad, reg_t, state, label, anchors)
    with pytest.raises(ValueError, match="row order"):
        tr._classification_torch(out, reg_t, state, label, anchors[:-9])
    with pytest.raises(ValueError, match="row order"):
        tr._classification_fwd_bwd(bad, reg_t, state, label, npos, anchors)


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_checkpoint_records_the_loss(tmp_path, ext):
    for kind in KINDS:
        tr = _trainer(classification_loss=kind)
        cfg = checkpoint.training_config(tr.base_optimizer)
        assert cfg["loss"] == {"regression": "_smooth_l1", "classification": "_" + kind}
        path = str(tmp_path / "{}.{}".format(kind, ext))
        checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
        assert checkpoint.stored_classification_loss(path) == kind
        assert checkpoint.stored_regression_loss(path) == "smooth_l1"
    plain = _trainer()
    path = str(tmp_path / ("plain." + ext))
    checkpoint.save_checkpoint(path, plain.model, plain.base_optimizer, epoch=1)
    assert checkpoint.stored_classification_loss(path) == "focal"
    weights_only = str(tmp_path / ("weights." + ext))
    checkpoint.save_checkpoint(weights_only, plain.model, None)
    assert checkpoint.stored_classification_loss(weights_only) is None


def test_default_training_config_is_unchanged():
    """Without the new argument the stored training_config is, byte for byte, the one written before it existed."""
    for tr in (_trainer(), _trainer(classification_loss="focal")):
        opt = tr.base_optimizer
        before = json.dumps({"optimizer_config": {"class_name": "Adam", "config": opt.get_config()},
                             "loss": {"regression": "_smooth_l1", "classification": "_focal"},
                             "metrics": [], "sample_weight_mode": None, "loss_weights": None})
        assert json.dumps(checkpoint.training_config(opt)) == before
    assert json.dumps(checkpoint.training_config(None)) == json.dumps(
        {"optimizer_config": {"class_name": "Adam", "config": {}},
         "loss": {"regression": "_smooth_l1", "classification": "_focal"},
         "metrics": [], "sample_weight_mode": None, "loss_weights": None})


# ------------------------------------------------------------------------------------------------ CLI
def test_flags_parse():
    a = T.parse_args(["coco", "/x"])
    assert a.classification_loss == "focal"
    for kind in KINDS:
        assert T.parse_args(["--classification-loss", kind, "coco", "/x"]).classification_loss == kind
    assert T.build_parser().get_default("classification_loss") is None
    with pytest.raises(SystemExit):
        T.parse_args(["--classification-loss", "gfl", "coco", "/x"])
    with pytest.raises(SystemExit, match="fp8"):
        T.parse_args(["--classification-loss", "qfl", "--dtype", "fp8", "coco", "/x"])
    assert T.parse_args(["--classification-loss", "focal", "--dtype", "fp8", "coco", "/x"]).dtype == "fp8"
    assert "--classification-loss" in T.build_parser().format_help() and "--classification-loss" in T.__doc__


def test_flags_against_snapshot(tmp_path, recwarn):
    tr = _trainer(classification_loss="vfl")
    path = str(tmp_path / "vfl.h5")
    checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
    a = T.parse_args(["--snapshot", path, "coco", "/x"])                     # the file decides
    assert a.classification_loss == "vfl"
    a = T.parse_args(["--snapshot", path, "--classification-loss", "vfl", "coco", "/x"])
    assert a.classification_loss == "vfl"
    assert not [w for w in recwarn.list if "classification-loss" in str(w.message)]
    with pytest.warns(UserWarning, match="classification-loss qfl differs.*vfl"):   # the flag wins
        a = T.parse_args(["--snapshot", path, "--classification-loss", "qfl", "coco", "/x"])
    assert a.classification_loss == "qfl"
    with pytest.warns(UserWarning, match="classification-loss focal differs"):
        a = T.parse_args(["--snapshot", path, "--classification-loss", "focal", "coco", "/x"])
    assert a.classification_loss == "focal"
    with pytest.raises(SystemExit, match="fp8"):                              # the stored loss is refused too
        T.parse_args(["--snapshot", path, "--dtype", "fp8", "coco", "/x"])


def test_cli_trains_snapshots_and_resumes(tmp_path):
    common = ["--no-weights", "--backbone", "resnet18", "--batch-size", "2", "--image-min-side", "64",
              "--image-max-side", "96", "--snapshot-path", str(tmp_path / "snap"), "--tensorboard-dir", "",
              "--device", "cpu", "--workers", "1", "--seed", "1", "--no-evaluation", "--lr", "1e-4"]
    data = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "4", "--max-boxes", "3"]
    h = T.main(common + ["--classification-loss", "qfl", "--epochs", "1", "--steps", "2"] + data)
    assert len(h.history["loss"]) == 1 and all(math.isfinite(v) for v in h.history["classification_loss"])
    ck = str(tmp_path / "snap" / "checkpoint-01.h5")
    assert os.path.exists(ck) and checkpoint.stored_classification_loss(ck) == "qfl"
    # resume without the flag: the snapshot says qfl, and the next snapshot says so again
    h2 = T.main(["--snapshot", ck] + common[1:] + ["--epochs", "2", "--steps", "1"] + data)
    assert h2.epoch == [1]
    assert checkpoint.stored_classification_loss(str(tmp_path / "snap" / "checkpoint-02.h5")) == "qfl"
