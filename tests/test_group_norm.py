"""``--head-norm gn`` without a GPU: the torch expression (``ops.norm``), the model wiring, the Trainer, checkpoints
and the flags.  The kernels are checked in test_group_norm_gpu.py."""
import json
import math
import os
import warnings

import pytest
import torch

from batchai_retinanet_horovod_coco_amd import models
from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.io import checkpoint
from batchai_retinanet_horovod_coco_amd.models.layers import GroupNorm
from batchai_retinanet_horovod_coco_amd.ops import norm as norm_ops

S = [(37, 41), (5, 7), (3, 4), (2, 2), (1, 1)]
NPIX = [h * w for h, w in S]
P = sum(NPIX)
B = 3
EPS = 1e-5


def _inputs(C=16, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, P, C, generator=g) * 1.5 + 0.3).to(dtype)
    gamma = (1 + 0.5 * torch.randn(C, generator=g)).to(dtype)
    beta = (0.3 * torch.randn(C, generator=g)).to(dtype)
    return x, gamma, beta


# ------------------------------------------------------------------------------------------------ the torch expression
@pytest.mark.parametrize("b,l,g", [(0, 0, 0), (2, 1, 1), (1, 4, 1), (2, 3, 0)])
def test_expression_against_a_hand_written_loop(b, l, g):
    C, G = 16, 2
    x, gamma, beta = _inputs(C)
    y = norm_ops.group_norm_relu_packed(x, S, gamma, beta, G, EPS)
    cpg, off, n = C // G, sum(NPIX[:l]), NPIX[l]
    vals = [float(x[b, off + r, g * cpg + c]) for r in range(n) for c in range(cpg)]
    mean = math.fsum(vals) / len(vals)
    var = math.fsum((v - mean) ** 2 for v in vals) / len(vals)
    rstd = 1.0 / math.sqrt(var + EPS)
    for r in range(n):
        for c in range(cpg):
            ch = g * cpg + c
            want = max(0.0, float(gamma[ch]) * (float(x[b, off + r, ch]) - mean) * rstd + float(beta[ch]))
            assert abs(float(y[b, off + r, ch]) - want) <= 1e-12 * max(1.0, abs(want))


def test_gradcheck_away_from_the_kink():
    C, G, shapes = 8, 2, [(3, 2), (1, 2), (1, 1)]
    g = torch.Generator().manual_seed(17)     # chosen so that every pre-activation is away from 0 (asserted below)
    x = torch.randn(2, 9, C, generator=g, dtype=torch.float64)
    gamma = 1 + 0.5 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    # the one-pixel level has 4 elements per group: its normalised values are far from 0 or pushed there by beta
    with torch.no_grad():
        pre = _pre(x, shapes, gamma, beta, G)
        assert float(pre.abs().min()) > 1e-3
    args = (x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True))
    assert torch.autograd.gradcheck(lambda a, b_, c: norm_ops.group_norm_relu_packed(a, shapes, b_, c, G, EPS), args,
                                    eps=1e-7, atol=1e-6)


def _pre(x, shapes, gamma, beta, G):
    out, off = [], 0
    for h, w in shapes:
        n = h * w
        v = x[:, off:off + n].reshape(x.shape[0], n, G, -1)
        m = v.mean(dim=(1, 3), keepdim=True)
        var = ((v - m) ** 2).mean(dim=(1, 3), keepdim=True)
        out.append(((v - m) / torch.sqrt(var + EPS)).reshape(x.shape[0], n, -1) * gamma + beta)
        off += n
    return torch.cat(out, 1)


def test_statistics_are_per_image_and_per_level():
    C, G = 16, 2
    x, gamma, beta = _inputs(C)
    y = norm_ops.group_norm_relu_packed(x, S, gamma, beta, G, EPS)
    x2 = x.clone()
    x2[1, NPIX[0]:NPIX[0] + NPIX[1]] += 5.0             # image 1, level 1
    y2 = norm_ops.group_norm_relu_packed(x2, S, gamma, beta, G, EPS)
    same = torch.ones(B, P, dtype=torch.bool)
    same[1, NPIX[0]:NPIX[0] + NPIX[1]] = False
    assert torch.equal(y[same], y2[same]) and not torch.equal(y[~same], y2[~same])
    # a level on its own is F.group_norm of its [B, C, h, w] tensor
    h, w = S[1]
    lv = x[:, NPIX[0]:NPIX[0] + NPIX[1]].reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous()
    want = torch.relu(torch.nn.functional.group_norm(lv, G, gamma, beta, EPS)).permute(0, 2, 3, 1).reshape(B, h * w, C)
    assert torch.equal(y[:, NPIX[0]:NPIX[0] + NPIX[1]], want)
    # 16-bit activations: fp32 arithmetic, the input's dtype out
    yb = norm_ops.group_norm_relu_packed(x.bfloat16(), S, gamma.float(), beta.float(), G, EPS)
    assert yb.dtype == torch.bfloat16 and torch.allclose(yb.double(), y, rtol=2 ** -7, atol=2 ** -7)
    with pytest.raises(ValueError, match="rows"):
        norm_ops.group_norm_relu_packed(x[:, :-1], S, gamma, beta, G, EPS)


# ------------------------------------------------------------------------------------------------ model
def _model(head_norm="gn", classes=3, seed=0, **kw):
    torch.manual_seed(seed)
    return models.backbone("resnet18").retinanet(classes, **(dict(head_norm=head_norm, **kw) if head_norm else {}))


def test_model_parameters_names_and_initial_values():
    plain, gn = _model(None), _model("gn")
    extra = [(n, p) for n, p in gn.named_parameters() if n not in dict(plain.named_parameters())]
    assert len(extra) == 16 and sum(p.numel() for _, p in extra) == 16 * 256
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in gn.named_parameters() if ".norms." not in n]
    assert plain.head_norm is None and gn.head_norm == "gn" and gn.head_norm_groups == 32
    assert plain.norms() == [] and len(gn.norms()) == 8
    for sub, prefix in ((gn.regression_submodel, "pyramid_regression"),
                        (gn.classification_submodel, "pyramid_classification")):
        for i, n in enumerate(sub.norms):
            assert isinstance(n, GroupNorm) and n.keras_name == "{}_{}_gn".format(prefix, i)
            assert n.groups == 32 and n.eps == 1e-5
            assert torch.equal(n.gamma, torch.ones(256)) and torch.equal(n.beta, torch.zeros(256))
            assert n.gamma.requires_grad and n.beta.requires_grad
    # the convs, their biases and their initial values are the plain model's (same seed)
    sd = plain.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in gn.state_dict().items() if k in sd) and set(sd) <= set(gn.state_dict())
    assert models.backbone("resnet18").retinanet(3, head_norm="gn", head_norm_groups=16).norms()[0].groups == 16
    assert models.backbone("resnet18").retinanet(3, head_norm="none").head_norm is None
    with pytest.raises(ValueError, match="head_norm"):
        _model("bn")
    with pytest.raises(ValueError, match="divide"):
        _model("gn", head_norm_groups=48)
    with pytest.raises(TypeError):
        models.backbone("resnet18").retinanet(3, head_normalisation="gn")


def test_wiring_equals_the_plain_model_with_identity_norms(monkeypatch):
    """Every GN replaced by its affine identity (ReLU kept): the GN model computes what the plain model computes."""
    plain, gn = _model(None), _model("gn")
    monkeypatch.setattr(norm_ops, "group_norm_relu_nhwc", lambda t, gamma, beta, groups, eps=1e-5: torch.relu(
        t * gamma.to(t.dtype) + beta.to(t.dtype)))
    x = torch.randn(2, 64, 96, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        a, b = plain(x), gn(x)
    assert torch.equal(a["regression"], b["regression"]) and torch.equal(a["classification"], b["classification"])
    monkeypatch.undo()
    with torch.no_grad():
        c = gn(x)
    assert not torch.equal(a["classification"], c["classification"])


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(head_norm="gn", seed=0, **kw):
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    return Trainer(_model(head_norm, seed=seed), lr=1e-3, clipnorm=0.0, device=torch.device("cpu"), **kw)


def _batch():
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    return make_batch(1, 64, 96, num_classes=3, max_boxes=3, generator=torch.Generator().manual_seed(5))


def _gn_segments(tr):
    return [s for s in tr.flat.segments if ".norms." in s.name]


def test_a_step_changes_gamma_and_beta():
    tr, b = _trainer(), _batch()
    logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    assert all(math.isfinite(float(v)) for v in logs.values())
    assert len(_gn_segments(tr)) == 16
    for n in tr.model.norms():
        assert not torch.equal(n.gamma, torch.ones(256)) and not torch.equal(n.beta, torch.zeros(256))


def test_sgd_decay_skips_the_norms():
    tr = _trainer(optimizer="sgd", momentum=0.9, weight_decay=1e-2)
    table = tr.base_optimizer.segment_decay()
    assert len(table) == len(tr.flat.segments)
    for s, wd in zip(tr.flat.segments, table):
        if ".norms." in s.name:
            assert wd == 0.0, s.name
        elif s.name.endswith("tower.0.weight"):
            assert wd == 1e-2
    assert sum(1 for s in tr.flat.segments if ".norms." in s.name) == 16


def test_ema_covers_the_norms():
    tr, b = _trainer(ema_decay=0.5), _batch()
    for _ in range(2):
        tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    opt = tr.base_optimizer
    for s in _gn_segments(tr):
        avg, w = opt.ema[s.offset:s.offset + s.numel], tr.flat.data[s.offset:s.offset + s.numel]
        init = 1.0 if s.name.endswith("gamma") else 0.0
        assert not torch.equal(avg, torch.full_like(avg, init)) and not torch.equal(avg, w)


def test_trainer_refuses_fp8(monkeypatch):
    from batchai_retinanet_horovod_coco_amd.ops import fp8
    tr = _trainer()
    monkeypatch.setattr(fp8, "enabled", lambda: True)
    with pytest.raises(ValueError, match="fp8"):
        _trainer()
    assert _trainer(None) is not None               # towers without the norm still go with fp8
    with pytest.raises(RuntimeError, match="fp8"):  # switched on after the constructor's check
        tr._classification_fwd_bwd({"classification": None}, None, None, None, None, None)


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_checkpoint_round_trip(tmp_path, ext, optimizer):
    kw = dict(optimizer="sgd", momentum=0.9) if optimizer == "sgd" else {}
    tr, b = _trainer(ema_decay=0.9, **kw), _batch()
    for _ in range(2):
        tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    path = str(tmp_path / ("gn." + ext))
    checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
    cfg = checkpoint.read_model_config(path)["config"]
    assert cfg["head_norm"] == "gn" and cfg["head_norm_groups"] == 32
    assert checkpoint.stored_head_norm(path) == ("gn", 32)
    assert [l for l in cfg["layers"] if l.endswith("_gn")] == [
        "pyramid_{}_{}_gn".format(p, i) for p in ("regression", "classification") for i in range(4)]
    if ext == "h5":
        from batchai_retinanet_horovod_coco_amd.io import hdf5
        g = hdf5.File(path, "r")["model_weights"]["pyramid_classification_2_gn"]
        assert hdf5.load_attributes_from_hdf5_group(g, "weight_names") == [
            "pyramid_classification_2_gn/gamma:0", "pyramid_classification_2_gn/beta:0"]
    model = models.load_model(path)
    assert model.head_norm == "gn" and len(model.norms()) == 8
    for (k, v), (k2, v2) in zip(tr.model.state_dict().items(), model.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    tr2 = _trainer(seed=1, ema_decay=0.9, **kw)
    tr2.model.load_state_dict(model.state_dict())
    assert checkpoint.load_optimizer(tr2.model, tr2.base_optimizer, path)
    o1, o2 = tr.base_optimizer, tr2.base_optimizer
    assert o1.iterations == o2.iterations
    for k, t in o1.state_tensors().items():
        assert torch.equal(t, o2.state_tensors()[k]), k
    seg = _gn_segments(tr)[0]
    slot = next(iter(o1.state_tensors().values()))
    assert slot[seg.offset:seg.offset + seg.numel].any()        # the norms' slots are in there


def test_default_config_is_unchanged():
    plain = _model(None)
    before = {"class_name": "RetinaNet", "framework": checkpoint.FRAMEWORK,
              "config": {"name": "retinanet", "backbone": plain.backbone_name, "num_classes": plain.num_classes,
                         "num_anchors": plain.num_anchors, "layers": list(checkpoint.keras_layers(plain).keys())}}
    assert json.dumps(checkpoint.model_config(plain)) == json.dumps(before)
    assert not [l for l in before["config"]["layers"] if l.endswith("_gn")]
    assert [k for k in plain.state_dict() if "norms" in k] == []


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_cross_loading(tmp_path, ext):
    plain, gn = _model(None, seed=1), _model("gn", seed=2)
    with torch.no_grad():
        for n in gn.norms():
            n.gamma.fill_(1.5)
    p_plain, p_gn = str(tmp_path / ("plain." + ext)), str(tmp_path / ("gn." + ext))
    checkpoint.save_checkpoint(p_plain, plain, None)
    checkpoint.save_checkpoint(p_gn, gn, None)
    # a file without the GN layers into a GN model: everything else loads, gamma / beta stay, one warning
    target = _model("gn", seed=3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        checkpoint.load_weights(target, p_plain, by_name=True)
    assert len([w for w in rec if "GroupNorm" in str(w.message)]) == 1
    assert torch.equal(target.regression_submodel.tower[0].weight, plain.regression_submodel.tower[0].weight)
    assert all(torch.equal(n.gamma, torch.ones(256)) and torch.equal(n.beta, torch.zeros(256)) for n in target.norms())
    # a file with them into a model without the norm
    with pytest.raises(ValueError, match="--head-norm"):
        checkpoint.load_weights(_model(None, seed=3), p_gn, by_name=True)
    # and the matching pair
    target = _model("gn", seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        checkpoint.load_weights(target, p_gn, by_name=True)
    assert all(torch.equal(n.gamma, torch.full((256,), 1.5)) for n in target.norms())


# ------------------------------------------------------------------------------------------------ CLI
def test_flags_parse():
    a = T.parse_args(["coco", "/x"])
    assert a.head_norm is None and a.head_norm_groups == 32 and T.head_norm_kwargs(a) == {}
    assert T.build_parser().get_default("head_norm") is None
    a = T.parse_args(["--head-norm", "none", "coco", "/x"])
    assert a.head_norm is None and T.head_norm_kwargs(a) == {}
    a = T.parse_args(["--head-norm", "gn", "coco", "/x"])
    assert T.head_norm_kwargs(a) == dict(head_norm="gn", head_norm_groups=32)
    a = T.parse_args(["--head-norm", "gn", "--head-norm-groups", "16", "coco", "/x"])
    assert T.head_norm_kwargs(a) == dict(head_norm="gn", head_norm_groups=16)
    with pytest.raises(SystemExit):
        T.parse_args(["--head-norm", "bn", "coco", "/x"])
    with pytest.raises(SystemExit, match="head-norm-groups goes with"):
        T.parse_args(["--head-norm-groups", "16", "coco", "/x"])
    with pytest.raises(SystemExit, match="head-norm-groups goes with"):
        T.parse_args(["--head-norm", "none", "--head-norm-groups", "16", "coco", "/x"])
    with pytest.raises(SystemExit, match="divide"):
        T.parse_args(["--head-norm", "gn", "--head-norm-groups", "48", "coco", "/x"])
    with pytest.raises(SystemExit, match="fp8"):
        T.parse_args(["--head-norm", "gn", "--dtype", "fp8", "coco", "/x"])
    assert T.parse_args(["--head-norm", "none", "--dtype", "fp8", "coco", "/x"]).dtype == "fp8"
    assert "--head-norm" in T.build_parser().format_help() and "--head-norm" in T.__doc__


def test_flags_against_snapshot(tmp_path, recwarn):
    path, plain = str(tmp_path / "gn.h5"), str(tmp_path / "plain.h5")
    checkpoint.save_checkpoint(path, _model("gn", head_norm_groups=16), None)
    checkpoint.save_checkpoint(plain, _model(None), None)
    a = T.parse_args(["--snapshot", path, "coco", "/x"])                     # the file decides
    assert (a.head_norm, a.head_norm_groups, a.head_norm_override) == ("gn", 16, False)
    a = T.parse_args(["--snapshot", path, "--head-norm", "gn", "coco", "/x"])
    assert (a.head_norm, a.head_norm_groups, a.head_norm_override) == ("gn", 16, False)
    a = T.parse_args(["--snapshot", plain, "coco", "/x"])
    assert (a.head_norm, a.head_norm_override) == (None, False)
    assert not [w for w in recwarn.list if "head-norm" in str(w.message)]
    with pytest.warns(UserWarning, match="head-norm none differs.*gn"):      # the flag wins
        a = T.parse_args(["--snapshot", path, "--head-norm", "none", "coco", "/x"])
    assert (a.head_norm, a.head_norm_override) == (None, True)
    with pytest.warns(UserWarning, match="head-norm gn differs.*none"):
        a = T.parse_args(["--snapshot", plain, "--head-norm", "gn", "coco", "/x"])
    assert (a.head_norm, a.head_norm_groups, a.head_norm_override) == ("gn", 32, True)
    with pytest.warns(UserWarning, match="head-norm-groups 32 differs"):
        a = T.parse_args(["--snapshot", path, "--head-norm-groups", "32", "coco", "/x"])
    assert (a.head_norm, a.head_norm_groups, a.head_norm_override) == ("gn", 32, True)
    with pytest.raises(SystemExit, match="fp8"):                              # the stored norm is refused too
        T.parse_args(["--snapshot", path, "--dtype", "fp8", "coco", "/x"])
    # the models the overrides build
    with pytest.warns(UserWarning, match="GroupNorm"):
        m = models.load_model(plain, head_norm="gn", head_norm_groups=32)
    assert m.head_norm == "gn"
    m = models.load_model(path, head_norm=None)
    assert m.head_norm is None and m.norms() == []


@pytest.mark.parametrize("first,second", [("gn", "none"), ("none", "gn")])
def test_cli_resumes_with_a_differing_flag(tmp_path, first, second):
    """The flag wins over an h5 snapshot in both directions: the weights both models have are loaded, the optimizer
    state (slots matched by position to another parameter list) is left fresh with a warning, and training goes on."""
    common = ["--no-weights", "--backbone", "resnet18", "--batch-size", "2", "--image-min-side", "64",
              "--image-max-side", "96", "--snapshot-path", str(tmp_path / "snap"), "--tensorboard-dir", "",
              "--device", "cpu", "--workers", "1", "--seed", "1", "--no-evaluation", "--lr", "1e-4"]
    data = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "4", "--max-boxes", "3"]
    T.main(common + ["--head-norm", first, "--epochs", "1", "--steps", "1"] + data)
    ck = str(tmp_path / "snap" / "checkpoint-01.h5")
    assert checkpoint.stored_head_norm(ck)[0] == (None if first == "none" else "gn")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        h = T.main(["--snapshot", ck] + common[1:] + ["--head-norm", second, "--epochs", "2", "--steps", "1"] + data)
    said = [str(w.message) for w in rec]
    assert any("head-norm {} differs".format(second) in m for m in said)
    assert any("optimizer state left fresh" in m for m in said)
    assert h.epoch == [1] and all(math.isfinite(v) for v in h.history["loss"])
    assert checkpoint.stored_head_norm(str(tmp_path / "snap" / "checkpoint-02.h5"))[0] == (
        None if second == "none" else "gn")


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_optimizer_state_of_another_parameter_list_is_left_fresh(tmp_path, ext):
    b = _batch()
    for src, dst in (("gn", None), (None, "gn")):
        tr = _trainer(src)
        tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
        path = str(tmp_path / "{}.{}".format(src, ext))
        checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
        other = _trainer(dst, seed=1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert not checkpoint.load_optimizer(other.model, other.base_optimizer, path) or ext == "safetensors"
        opt = other.base_optimizer
        assert opt.iterations == 0 and not opt.m.any() and not opt.v.any()


def test_cli_trains_snapshots_and_resumes(tmp_path):
    common = ["--no-weights", "--backbone", "resnet18", "--batch-size", "2", "--image-min-side", "64",
              "--image-max-side", "96", "--snapshot-path", str(tmp_path / "snap"), "--tensorboard-dir", "",
              "--device", "cpu", "--workers", "1", "--seed", "1", "--no-evaluation", "--lr", "1e-4"]
    data = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "4", "--max-boxes", "3"]
    h = T.main(common + ["--head-norm", "gn", "--epochs", "1", "--steps", "2"] + data)
    assert len(h.history["loss"]) == 1 and all(math.isfinite(v) for v in h.history["loss"])
    ck = str(tmp_path / "snap" / "checkpoint-01.h5")
    assert os.path.exists(ck) and checkpoint.stored_head_norm(ck) == ("gn", 32)
    # resume without the flag: the snapshot's model has the norm, and the next snapshot says so again
    h2 = T.main(["--snapshot", ck] + common[1:] + ["--epochs", "2", "--steps", "1"] + data)
    assert h2.epoch == [1]
    assert checkpoint.stored_head_norm(str(tmp_path / "snap" / "checkpoint-02.h5")) == ("gn", 32)
