"""``--regression-bins`` without a GPU: the torch expressions (``ops.boxes.box_integral``,
``ops.losses.distribution_focal_loss``), the model wiring, the Trainer, checkpoints and the flags.  The kernels are
checked in test_box_dist_gpu.py."""
import json
import math
import os
import warnings

import pytest
import torch

from batchai_retinanet_horovod_coco_amd import models
from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.io import checkpoint
from batchai_retinanet_horovod_coco_amd.ops import boxes as box_ops
from batchai_retinanet_horovod_coco_amd.ops import losses


def _inputs(K, rows=12, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(2, rows, 4 * K, generator=g) * 2).to(dtype)
    reg_t = (torch.randn(2, rows, 4, generator=g) * 3).to(dtype)
    state = torch.randint(-1, 2, (2, rows), generator=g).to(torch.int8)
    state[0, 0] = 1
    return logits, reg_t, state


# ------------------------------------------------------------------------------------------------ the torch expressions
def test_bins():
    assert box_ops.box_bins(17, 8.0, torch.float64).tolist() == [float(i) for i in range(-8, 9)]
    v = box_ops.box_bins(5, 3.0, torch.float64)
    assert v.tolist() == [-3.0, -1.5, 0.0, 1.5, 3.0]
    for bad in (1, 33, -2):
        with pytest.raises(ValueError, match="regression_bins"):
            box_ops.check_regression_bins(bad)
    with pytest.raises(ValueError, match="regression_range"):
        box_ops.check_regression_bins(17, 0.0)
    assert box_ops.check_regression_bins(0) == (0, 8.0) and box_ops.check_regression_bins(None) == (0, 8.0)


@pytest.mark.parametrize("K,R", [(17, 8.0), (8, 8.0), (5, 3.0)])
def test_integral_against_a_hand_written_loop(K, R):
    logits, _, _ = _inputs(K)
    y = box_ops.box_integral(logits, K, R)
    assert y.shape == (2, 12, 4) and y.dtype == torch.float64
    D = 2 * R / (K - 1)
    for b, r, s in [(0, 0, 0), (1, 11, 3), (0, 5, 2), (1, 3, 1)]:
        l = [float(logits[b, r, s * K + i]) for i in range(K)]
        m = max(l)
        e = [math.exp(x - m) for x in l]
        S = math.fsum(e)
        want = math.fsum(e[i] / S * (-R + i * D) for i in range(K))
        assert abs(float(y[b, r, s]) - want) <= 1e-12 * max(1.0, abs(want))


def _dfl_loop(logits, reg_t, state, K, R, weight):
    D = 2 * R / (K - 1)
    total, npos = [], 0
    B, A = state.shape
    for b in range(B):
        for r in range(A):
            if int(state[b, r]) != 1:
                continue
            npos += 1
            for s in range(4):
                l = [float(logits[b, r, s * K + i]) for i in range(K)]
                m = max(l)
                lse = m + math.log(math.fsum(math.exp(x - m) for x in l))
                u = min(max((float(reg_t[b, r, s]) + R) / D, 0.0), (K - 1) - 0.01)
                il = math.floor(u)
                wr = u - il
                total.append(-((1 - wr) * (l[il] - lse) + wr * (l[il + 1] - lse)))
    return weight * math.fsum(total) / (4 * max(1, npos))


@pytest.mark.parametrize("K,R", [(17, 8.0), (8, 8.0), (5, 3.0)])
def test_dfl_against_a_hand_written_loop(K, R):
    logits, reg_t, state = _inputs(K)
    got = losses.distribution_focal_loss(logits, reg_t, state, K, R, 0.25)
    want = _dfl_loop(logits, reg_t, state, K, R, 0.25)
    assert got.dtype == torch.float64 and abs(float(got) - want) <= 1e-12 * abs(want)
    assert abs(float(losses.distribution_focal_loss(logits, reg_t, state, K, R, 1.0)) - 4 * want) <= 1e-11 * abs(want)


def test_gradcheck_integral():
    logits = _inputs(5, rows=3)[0].requires_grad_(True)
    assert torch.autograd.gradcheck(lambda l: box_ops.box_integral(l, 5, 3.0), (logits,))
    # the stated backward: dl_i = g p_i (v_i - y)
    g = torch.randn(2, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    (dl,) = torch.autograd.grad(box_ops.box_integral(logits, 5, 3.0), logits, g)
    p = torch.softmax(logits.detach().reshape(2, 3, 4, 5), -1)
    v = box_ops.box_bins(5, 3.0, torch.float64)
    y = (p * v).sum(-1, keepdim=True)
    assert torch.allclose(dl.reshape(2, 3, 4, 5), g[..., None] * p * (v - y), rtol=1e-12, atol=1e-14)


def test_gradcheck_dfl_away_from_the_clamp_ends():
    K, R = 5, 3.0
    logits, reg_t, state = _inputs(K, rows=3)
    reg_t = reg_t.clamp(-2.9, 2.9)
    assert torch.autograd.gradcheck(
        lambda l: losses.distribution_focal_loss(l, reg_t, state, K, R, 0.25), (logits.requires_grad_(True),))
    # the stated gradient: p_i - wl [i == il] - wr [i == il + 1], over 4 max(1, npos), times the weight
    (dl,) = torch.autograd.grad(losses.distribution_focal_loss(logits, reg_t, state, K, R, 0.25), logits)
    p = torch.softmax(logits.detach().reshape(2, 3, 4, K), -1)
    u = (reg_t + R) / (2 * R / (K - 1))
    il = u.floor().long()
    want = p.clone()
    want.scatter_add_(-1, il[..., None], -(1 - (u - il))[..., None])
    want.scatter_add_(-1, il[..., None] + 1, -(u - il)[..., None])
    pos = (state == 1)
    want = want * pos[..., None, None] * 0.25 / (4 * max(1, int(pos.sum())))
    assert torch.allclose(dl.reshape(2, 3, 4, K), want, rtol=1e-12, atol=1e-15)


def test_targets_on_a_bin_and_beyond_the_range():
    K, R = 17, 8.0
    logits = _inputs(K, rows=1)[0][:1].clone().requires_grad_(True)      # (1, 1, 68)
    state = torch.ones(1, 1, dtype=torch.int8)
    logp = torch.log_softmax(logits.detach().reshape(4, K), -1)
    # exactly on bin values: all the weight on that bin
    t = torch.tensor([[[-8.0, 0.0, 3.0, 7.0]]], dtype=torch.float64)
    got = losses.distribution_focal_loss(logits, t, state, K, R, 1.0)
    want = -(logp[0, 0] + logp[1, 8] + logp[2, 11] + logp[3, 15]) / 4
    assert abs(float(got.detach()) - float(want)) <= 1e-12
    # beyond both ends: the lower end is bin 0, the upper end 0.01 of a bin below the last value
    t = torch.tensor([[[-20.0, 30.0, -8.0 - 1e-9, 8.0]]], dtype=torch.float64)
    got = losses.distribution_focal_loss(logits, t, state, K, R, 1.0)
    hi = -(0.01 * logp[:, 15] + 0.99 * logp[:, 16])
    want = (-logp[0, 0] + hi[1] - logp[2, 0] + hi[3]) / 4
    assert abs(float(got.detach()) - float(want)) <= 1e-12
    (dl,) = torch.autograd.grad(got, logits)
    assert torch.isfinite(dl).all() and dl.abs().max() <= 0.25
    # the loss is continuous where u crosses an integer
    lo = losses.distribution_focal_loss(logits, torch.full((1, 1, 4), 3.0 - 1e-9, dtype=torch.float64), state, K, R)
    up = losses.distribution_focal_loss(logits, torch.full((1, 1, 4), 3.0 + 1e-9, dtype=torch.float64), state, K, R)
    assert abs(float(lo.detach()) - float(up.detach())) <= 1e-8


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
def test_logits_of_plus_minus_80(dtype):
    K, R = 17, 8.0
    logits = torch.zeros(1, 2, 4 * K, dtype=dtype)
    logits[0, 0, 3] = 80.0           # side 0: all the mass on bin 3 -> v = -5
    logits[0, 0, K:2 * K] = -80.0    # side 1: all equal -> the mean of the bins, 0
    logits[0, 0, 2 * K + 16] = -80.0
    logits[0, 1, 5] = 80.0
    logits[0, 1, 6] = -80.0
    y = box_ops.box_integral(logits, K, R)
    assert y.dtype == dtype and torch.isfinite(y.float()).all()
    assert float(y[0, 0, 0]) == -5.0 and float(y[0, 1, 0]) == -3.0
    assert abs(float(y[0, 0, 1])) <= 1e-5                # 17 products of 1/17 (rounded) with the integers -8..8
    assert abs(float(y[0, 0, 2]) + 0.5) <= (2 ** -8 if dtype == torch.bfloat16 else 1e-6)   # bins -8..7: mean -0.5
    l = logits.clone().requires_grad_(True)
    state = torch.ones(1, 2, dtype=torch.int8)
    t = torch.tensor([[[-5.0, 0.3, 8.0, -8.0], [2.0, -2.0, 0.0, 0.5]]])
    loss = losses.distribution_focal_loss(l, t, state, K, R, 0.25)
    (dl,) = torch.autograd.grad(loss, l)
    assert math.isfinite(float(loss)) and torch.isfinite(dl.float()).all()
    # side (0, 2): the target 8 sits on the bin whose logit is -80 -> about 0.99 * 80 of loss on that side
    assert float(loss) > 0.25 * 0.99 * 80 / 8


def test_no_positives_gives_zero_loss_and_exactly_zero_gradient():
    K = 17
    logits, reg_t, state = _inputs(K)
    state = torch.where(state == 1, torch.zeros_like(state), state)
    l = logits.requires_grad_(True)
    loss = losses.distribution_focal_loss(l, reg_t, state, K, 8.0, 0.25)
    (dl,) = torch.autograd.grad(loss, l)
    assert float(loss) == 0.0 and not dl.any()


def test_expressions_refuse_wrong_shapes():
    with pytest.raises(ValueError, match="4 \\* K"):
        box_ops.box_integral(torch.zeros(2, 3, 60), 17)
    with pytest.raises(ValueError, match="4 \\* K"):
        losses.distribution_focal_loss(torch.zeros(2, 3, 60), torch.zeros(2, 3, 4), torch.zeros(2, 3), 17)


# ------------------------------------------------------------------------------------------------ model
def _model(bins=17, classes=3, seed=0, **kw):
    torch.manual_seed(seed)
    return models.backbone("resnet18").retinanet(classes, **(dict(regression_bins=bins, **kw) if bins else {}))


def test_model_parameters_and_default_model():
    plain, dist = _model(0), _model(17)
    assert plain.regression_bins == 0 and dist.regression_bins == 17 and dist.regression_range == 8.0
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in dist.named_parameters()]
    for (n, a), (_, b) in zip(plain.named_parameters(), dist.named_parameters()):
        if n.startswith("regression_submodel.final."):
            assert b.shape[0] == 17 * a.shape[0] == 9 * 4 * 17 and b.shape[1:] == a.shape[1:]
        else:
            assert a.shape == b.shape, n
    final = dist.regression_submodel.final
    assert final.keras_name == "pyramid_regression" and not final.bias.any()
    assert abs(float(final.weight.std()) - 0.01) < 1e-3          # normal(0, 0.01) like the plain final
    assert models.backbone("resnet18").retinanet(3, regression_bins=0).regression_bins == 0
    assert sum(p.numel() for p in models.backbone("resnet18").retinanet(3, regression_bins=0).parameters()) == \
        sum(p.numel() for p in plain.parameters())
    assert models.backbone("resnet18").retinanet(3, regression_bins=8, regression_range=4.0).regression_range == 4.0
    with pytest.raises(ValueError, match="regression_bins"):
        _model(33)
    with pytest.raises(ValueError, match="regression_bins"):
        _model(1)
    with pytest.raises(ValueError, match="regression_range"):
        _model(17, regression_range=-1.0)


def test_model_outputs_and_channel_order():
    K = 5
    m = _model(K, regression_range=3.0).eval()
    x = torch.randn(1, 64, 96, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        out = m(x)
    A = out["classification"].shape[1]
    assert out["regression_logits"].shape == (1, A, 4 * K) and out["regression"].shape == (1, A, 4)
    assert torch.equal(out["regression"], box_ops.box_integral(out["regression_logits"], K, 3.0))
    # one hot logit through the bias of channel a * 4K + s * K + i moves exactly delta (a, s) of every location to v_i
    v = box_ops.box_bins(K, 3.0)
    base = out["regression"].reshape(1, -1, 9, 4)
    for a, s, i in [(0, 0, 0), (4, 2, 3), (8, 3, 4)]:
        with torch.no_grad():
            m.regression_submodel.final.bias.zero_()
            m.regression_submodel.final.bias[a * 4 * K + s * K + i] = 60.0
            reg = m(x)["regression"].reshape(1, -1, 9, 4)
        hit = reg[:, :, a, s]
        assert torch.allclose(hit, torch.full_like(hit, float(v[i])), atol=1e-4)
        rest = reg.clone()
        rest[:, :, a, s] = base[:, :, a, s]
        assert torch.equal(rest, base)              # and no other
    # the prediction model reads the integral deltas
    with torch.no_grad():
        m.regression_submodel.final.bias.zero_()
        b, sc, lab = models.retinanet_bbox(m)(x)
    assert b.shape[-1] == 4 and b.shape[:2] == sc.shape == lab.shape
    # differentiable on the torch path
    m.train()
    out = m(x)
    out["regression"].sum().backward()
    assert m.regression_submodel.final.weight.grad.abs().sum() > 0


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(bins=17, seed=0, **kw):
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    return Trainer(_model(bins, seed=seed), lr=1e-3, clipnorm=0.0, device=torch.device("cpu"), **kw)


def _batch():
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    return make_batch(1, 64, 96, num_classes=3, max_boxes=3, generator=torch.Generator().manual_seed(5))


@pytest.mark.parametrize("kw", [dict(), dict(regression_loss="giou"), dict(regression_loss="diou"),
                                dict(regression_loss="ciou"),
                                dict(regression_loss="giou", classification_loss="qfl", assigner="atss")],
                         ids=["smooth_l1", "giou", "diou", "ciou", "giou-qfl-atss"])
def test_a_trainer_step(kw):
    tr, b = _trainer(**kw), _batch()
    w0 = tr.model.regression_submodel.final.weight.detach().clone()
    args = (b["images"], b["gt"], b["gt_count"], b["image_hw"])
    reg0, cls0 = tr.forward_losses(*args)
    logs = tr.train_on_batch(*args)
    assert set(logs) == {"loss", "regression_loss", "classification_loss"}       # no new log key
    assert all(math.isfinite(float(v)) for v in logs.values())
    assert abs(float(logs["regression_loss"]) - float(reg0)) <= 1e-5 * abs(float(reg0))
    assert not torch.equal(tr.model.regression_submodel.final.weight, w0)
    # the logged regression loss is the box loss on the integral deltas plus the DFL term
    plain = _trainer(**kw)
    plain.dfl_weight = 0.0
    box_only, _ = plain.forward_losses(*args)
    state, _, reg_t, _ = plain.compute_targets(*args)
    assert int((state == 1).sum()) > 0
    with torch.no_grad():
        out = plain.model(b["images"])
    dfl = losses.distribution_focal_loss(out["regression_logits"], reg_t, state, 17, 8.0, 0.25)
    assert float(dfl) > 0 and abs(float(reg0) - float(box_only) - float(dfl)) <= 1e-5 * abs(float(reg0))


def test_trainer_arguments():
    tr = _trainer(dfl_weight=0.5)
    assert tr.regression_bins == 17 and tr.dfl_weight == 0.5 and tr.base_optimizer.dfl_weight == 0.5
    assert checkpoint.training_config(tr.base_optimizer)["dfl_weight"] == 0.5
    assert "dfl_weight" not in checkpoint.training_config(_trainer().base_optimizer)
    assert _trainer(0).regression_bins == 0
    with pytest.raises(ValueError, match="dfl_weight goes with"):
        _trainer(0, dfl_weight=0.5)
    with pytest.raises(ValueError, match="dfl_weight must be"):
        _trainer(dfl_weight=-1.0)


def test_sgd_decays_the_final_like_any_conv_kernel():
    tr = _trainer(optimizer="sgd", momentum=0.9, weight_decay=1e-2)
    table = dict(zip((s.name for s in tr.flat.segments), tr.base_optimizer.segment_decay()))
    assert table["regression_submodel.final.weight"] == table["regression_submodel.tower.0.weight"] == 1e-2
    assert table["regression_submodel.final.bias"] == table["regression_submodel.tower.0.bias"]


def test_trainer_refuses_fp8(monkeypatch):
    from batchai_retinanet_horovod_coco_amd.ops import fp8
    tr = _trainer()
    monkeypatch.setattr(fp8, "enabled", lambda: True)
    with pytest.raises(ValueError, match="fp8"):
        _trainer()
    assert _trainer(0) is not None                  # the 4-number head still goes with fp8
    with pytest.raises(RuntimeError, match="fp8"):  # switched on after the constructor's check
        tr._dist_losses_fused({"regression_logits": None, "regression": None}, None, None, None, None, 9, None)


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_checkpoint_round_trip(tmp_path, ext, optimizer):
    kw = dict(optimizer="sgd", momentum=0.9) if optimizer == "sgd" else {}
    torch.manual_seed(0)
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    tr = Trainer(_model(8, regression_range=6.0), lr=1e-3, clipnorm=0.0, device=torch.device("cpu"), ema_decay=0.9,
                 dfl_weight=0.5, **kw)
    b = _batch()
    for _ in range(2):
        tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    path = str(tmp_path / ("dist." + ext))
    checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
    cfg = checkpoint.read_model_config(path)["config"]
    assert cfg["regression_bins"] == 8 and cfg["regression_range"] == 6.0
    assert checkpoint.stored_regression_bins(path) == (8, 6.0) and checkpoint.stored_dfl_weight(path) == 0.5
    model = models.load_model(path)
    assert model.regression_bins == 8 and model.regression_range == 6.0
    for (k, v), (k2, v2) in zip(tr.model.state_dict().items(), model.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    # the averaged set holds the wide final too
    ema = _model(8, seed=3, regression_range=6.0)
    checkpoint.load_weights(ema, path, group="ema_weights")
    f = ema.regression_submodel.final.weight
    assert f.shape[0] == 9 * 4 * 8 and not torch.equal(f, tr.model.regression_submodel.final.weight)
    tr2 = Trainer(_model(8, seed=1, regression_range=6.0), lr=1e-3, clipnorm=0.0, device=torch.device("cpu"),
                  ema_decay=0.9, dfl_weight=0.5, **kw)
    tr2.model.load_state_dict(model.state_dict())
    assert checkpoint.load_optimizer(tr2.model, tr2.base_optimizer, path)
    o1, o2 = tr.base_optimizer, tr2.base_optimizer
    assert o1.iterations == o2.iterations
    for k, t in o1.state_tensors().items():
        assert torch.equal(t, o2.state_tensors()[k]), k
    seg = tr.flat.by_param[id(tr.model.regression_submodel.final.weight)]
    for slot in o1.state_tensors().values():
        assert slot[seg.offset:seg.offset + seg.numel].any()        # the wide final's slots are in there


def test_default_files_are_unchanged():
    plain = _model(0)
    before = {"class_name": "RetinaNet", "framework": checkpoint.FRAMEWORK,
              "config": {"name": "retinanet", "backbone": plain.backbone_name, "num_classes": plain.num_classes,
                         "num_anchors": plain.num_anchors, "layers": list(checkpoint.keras_layers(plain).keys())}}
    assert json.dumps(checkpoint.model_config(plain)) == json.dumps(before)
    assert checkpoint.model_config(_model(17))["config"]["layers"] == before["config"]["layers"]
    tr = _trainer(0)
    assert "dfl_weight" not in checkpoint.training_config(tr.base_optimizer)
    assert plain.regression_submodel.final.weight.shape[0] == 36


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_cross_loading(tmp_path, ext):
    plain, dist = _model(0, seed=1), _model(17, seed=2)
    p_plain, p_dist = str(tmp_path / ("plain." + ext)), str(tmp_path / ("dist." + ext))
    checkpoint.save_checkpoint(p_plain, plain, None)
    checkpoint.save_checkpoint(p_dist, dist, None)
    for path, src, bins in ((p_plain, plain, 17), (p_dist, dist, 0), (p_dist, dist, 8)):
        # strict loading names the layer ...
        with pytest.raises(ValueError, match="pyramid_regression|regression_submodel"):
            checkpoint.load_weights(_model(bins, seed=3), path, by_name=True)
        # ... --weights (skip_mismatch) skips that one layer and loads every other
        target = _model(bins, seed=3)
        init = target.regression_submodel.final.weight.detach().clone()
        skipped = checkpoint.load_weights(target, path, by_name=True, skip_mismatch=True)
        assert len(skipped) == 2 and all("regression" in s for s in skipped)
        assert torch.equal(target.regression_submodel.final.weight, init)
        assert torch.equal(target.regression_submodel.tower[3].weight, src.regression_submodel.tower[3].weight)
        assert torch.equal(target.classification_submodel.final.weight, src.classification_submodel.final.weight)
        # load_model with the keyword: the same, with one warning
        torch.manual_seed(4)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            m = models.load_model(path, regression_bins=bins)
        assert len([w for w in rec if "regression final" in str(w.message)]) == 1
        assert m.regression_bins == bins and m.regression_submodel.final.weight.shape[0] == 36 * max(1, bins)
        assert torch.equal(m.regression_submodel.tower[0].weight, src.regression_submodel.tower[0].weight)
        assert torch.equal(m.fpn.P3.weight, src.fpn.P3.weight) and not m.regression_submodel.final.bias.any()
    # and the matching pair, without a warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = models.load_model(p_dist)
    assert torch.equal(m.regression_submodel.final.weight, dist.regression_submodel.final.weight)


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_optimizer_state_of_another_parameter_list_is_left_fresh(tmp_path, ext):
    b = _batch()
    for src, dst in ((17, 0), (0, 17)):
        tr = _trainer(src, ema_decay=0.9)
        tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
        path = str(tmp_path / "{}.{}".format(src, ext))
        checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
        other = _trainer(dst, seed=1, ema_decay=0.9)
        with pytest.warns(UserWarning, match="optimizer state left fresh"):
            assert not checkpoint.load_optimizer(other.model, other.base_optimizer, path)
        opt = other.base_optimizer
        assert opt.iterations == 0 and not opt.m.any() and not opt.v.any()


# ------------------------------------------------------------------------------------------------ CLI
def test_flags_parse():
    a = T.parse_args(["coco", "/x"])
    assert (a.regression_bins, a.regression_range, a.dfl_weight) == (0, 8.0, 0.25) and T.regression_bins_kwargs(a) == {}
    assert T.build_parser().get_default("regression_bins") is None
    a = T.parse_args(["--regression-bins", "0", "coco", "/x"])
    assert a.regression_bins == 0 and T.regression_bins_kwargs(a) == {}
    a = T.parse_args(["--regression-bins", "17", "coco", "/x"])
    assert T.regression_bins_kwargs(a) == dict(regression_bins=17, regression_range=8.0) and a.dfl_weight == 0.25
    a = T.parse_args(["--regression-bins", "8", "--regression-range", "4", "--dfl-weight", "0.5", "coco", "/x"])
    assert T.regression_bins_kwargs(a) == dict(regression_bins=8, regression_range=4.0) and a.dfl_weight == 0.5
    for bad in ("1", "33", "-3"):
        with pytest.raises(SystemExit, match="regression-bins must be"):
            T.parse_args(["--regression-bins", bad, "coco", "/x"])
    with pytest.raises(SystemExit, match="regression-range goes with"):
        T.parse_args(["--regression-range", "4", "coco", "/x"])
    with pytest.raises(SystemExit, match="dfl-weight goes with"):
        T.parse_args(["--regression-bins", "0", "--dfl-weight", "0.5", "coco", "/x"])
    with pytest.raises(SystemExit, match="regression-range must be"):
        T.parse_args(["--regression-bins", "17", "--regression-range", "0", "coco", "/x"])
    with pytest.raises(SystemExit, match="fp8"):
        T.parse_args(["--regression-bins", "17", "--dtype", "fp8", "coco", "/x"])
    assert T.parse_args(["--regression-bins", "0", "--dtype", "fp8", "coco", "/x"]).dtype == "fp8"
    assert "--regression-bins" in T.build_parser().format_help() and "--regression-bins" in T.__doc__
    assert "--dfl-weight" in T.__doc__ and "--regression-range" in T.__doc__


def test_flags_against_snapshot(tmp_path, recwarn):
    path, plain = str(tmp_path / "dist.h5"), str(tmp_path / "plain.h5")
    checkpoint.save_checkpoint(path, _model(8, regression_range=6.0), None)
    checkpoint.save_checkpoint(plain, _model(0), None)
    a = T.parse_args(["--snapshot", path, "coco", "/x"])                     # the file decides
    assert (a.regression_bins, a.regression_range, a.regression_bins_override) == (8, 6.0, False)
    a = T.parse_args(["--snapshot", path, "--regression-bins", "8", "coco", "/x"])
    assert (a.regression_bins, a.regression_range, a.regression_bins_override) == (8, 6.0, False)
    a = T.parse_args(["--snapshot", plain, "coco", "/x"])
    assert (a.regression_bins, a.regression_bins_override) == (0, False)
    assert not [w for w in recwarn.list if "regression-bins" in str(w.message)]
    with pytest.warns(UserWarning, match="regression-bins 0 differs.*8"):    # the flag wins
        a = T.parse_args(["--snapshot", path, "--regression-bins", "0", "coco", "/x"])
    assert (a.regression_bins, a.regression_bins_override) == (0, True)
    with pytest.warns(UserWarning, match="regression-bins 17 differs.*0"):
        a = T.parse_args(["--snapshot", plain, "--regression-bins", "17", "coco", "/x"])
    assert (a.regression_bins, a.regression_range, a.regression_bins_override) == (17, 8.0, True)
    with pytest.warns(UserWarning, match="regression-range 4.0 differs"):
        a = T.parse_args(["--snapshot", path, "--regression-range", "4", "coco", "/x"])
    assert (a.regression_bins, a.regression_range, a.regression_bins_override) == (8, 4.0, True)
    with pytest.raises(SystemExit, match="fp8"):                              # the stored head is refused too
        T.parse_args(["--snapshot", path, "--dtype", "fp8", "coco", "/x"])
    with pytest.raises(SystemExit, match="regression-range goes with"):
        T.parse_args(["--snapshot", plain, "--regression-range", "4", "coco", "/x"])


COMMON = ["--no-weights", "--backbone", "resnet18", "--batch-size", "2", "--image-min-side", "64",
          "--image-max-side", "96", "--tensorboard-dir", "", "--device", "cpu", "--workers", "1", "--seed", "1",
          "--no-evaluation", "--lr", "1e-4"]
DATA = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "4", "--max-boxes", "3"]


@pytest.mark.parametrize("first,second", [("17", "0"), ("0", "17")])
def test_cli_resumes_with_a_differing_flag(tmp_path, first, second):
    """The flag wins over an h5 snapshot in both directions: every layer but the regression final is loaded, the
    optimizer state (slots of another parameter list) is left fresh with a warning, and training goes on."""
    common = COMMON + ["--snapshot-path", str(tmp_path / "snap")]
    T.main(common + ["--regression-bins", first, "--epochs", "1", "--steps", "1"] + DATA)
    ck = str(tmp_path / "snap" / "checkpoint-01.h5")
    assert checkpoint.stored_regression_bins(ck)[0] == int(first)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        h = T.main(["--snapshot", ck] + common[1:] + ["--regression-bins", second, "--epochs", "2", "--steps", "1"]
                   + DATA)
    said = [str(w.message) for w in rec]
    assert any("regression-bins {} differs".format(second) in m for m in said)
    assert any("regression final" in m for m in said)
    assert any("optimizer state left fresh" in m for m in said)
    assert h.epoch == [1] and all(math.isfinite(v) for v in h.history["loss"])
    assert checkpoint.stored_regression_bins(str(tmp_path / "snap" / "checkpoint-02.h5"))[0] == int(second)


def test_cli_trains_snapshots_and_resumes(tmp_path):
    common = COMMON + ["--snapshot-path", str(tmp_path / "snap")]
    recipe = ["--regression-bins", "17", "--dfl-weight", "0.5", "--regression-loss", "giou", "--classification-loss",
              "qfl", "--assigner", "atss", "--head-norm", "gn"]
    h = T.main(common + recipe + ["--epochs", "1", "--steps", "2"] + DATA)
    assert len(h.history["loss"]) == 1 and all(math.isfinite(v) for v in h.history["loss"])
    ck = str(tmp_path / "snap" / "checkpoint-01.h5")
    assert os.path.exists(ck) and checkpoint.stored_regression_bins(ck) == (17, 8.0)
    assert checkpoint.stored_dfl_weight(ck) == 0.5
    # resume without the flags: the snapshot's model has the head and the stored weight, and the next snapshot says so
    h2 = T.main(["--snapshot", ck] + common[1:] + ["--epochs", "2", "--steps", "1"] + DATA)
    assert h2.epoch == [1]
    ck2 = str(tmp_path / "snap" / "checkpoint-02.h5")
    assert checkpoint.stored_regression_bins(ck2) == (17, 8.0) and checkpoint.stored_dfl_weight(ck2) == 0.5
