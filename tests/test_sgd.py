"""``KerasSGD`` (train/optimizer.py) on the CPU: the torch expression against a float64 evaluation of Keras 2
``SGD(lr, momentum, decay, nesterov)`` with coupled L2 weight decay on the rank >= 2 parameters, alone and through
``DistributedOptimizer``; SGD checkpoints in both formats, and Adam files unchanged; the ``train.py`` flags; Horovod's
momentum correction in the learning-rate callbacks."""
import glob
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.io import checkpoint, hdf5
from batchai_retinanet_horovod_coco_amd.parallel import callbacks as hvd_callbacks
from batchai_retinanet_horovod_coco_amd.parallel.distributed_optimizer import DistributedOptimizer
from batchai_retinanet_horovod_coco_amd.train.flat import FlatParams
from batchai_retinanet_horovod_coco_amd.train.optimizer import KerasAdam, KerasSGD

SHAPES = [(5, 3, 3, 2), (11,), (6, 7)]      # a conv kernel, a bias (rank 1: no decay), a rank-2 matrix
LR = 0.05
STEPS = 5
# the gradient norm is about sqrt(90 + 11 + 42) = 12: 0.5 clips every step, 1e6 never does, None is off
CLIPS = {"active": 0.5, "inactive": 1e6, "off": None}


def _f32(x):
    return float(np.float32(x))


def _flat(seed=0):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SHAPES]
    return FlatParams([(str(i), p) for i, p in enumerate(params)]), gen


def _grads(flat, gen, n=STEPS):
    pad = torch.ones(flat.total, dtype=torch.bool)
    for s in flat.segments:
        pad[s.offset:s.offset + s.numel] = False
    out = []
    for _ in range(n):
        g = torch.randn(flat.total, generator=gen)
        g[pad] = 0
        out.append(g)
    return out


def reference(flat, p0, grads, lr, momentum, nesterov, decay, weight_decay, clipnorm, world=1):
    """float64 evaluation of the update rule; returns (p, v, clip was active in every step / in no step)."""
    p, v = p0.double().clone(), torch.zeros(flat.total, dtype=torch.float64)
    wd = torch.zeros(flat.total, dtype=torch.float64)
    for s in flat.segments:
        if len(s.shape) >= 2:
            wd[s.offset:s.offset + s.numel] = _f32(weight_decay)
    clipped = []
    for i, g in enumerate(grads):
        g = g.double()
        norm = math.sqrt(float((g * g).sum()))
        f = 1.0
        if clipnorm and norm >= clipnorm:
            f = clipnorm / norm
        clipped.append(f != 1.0)
        lr_t = lr / (1.0 + decay * i)                    # t - 1 = i
        ge = g * (f / world) + wd * p
        v = momentum * v - lr_t * ge
        p = p + momentum * v - lr_t * ge if nesterov else p + v
    return p, v, clipped


def _close(got, want, what):
    # fp32 rounds to 2^-24 = 6e-8 relative; a step is at most 6 roundings per element and there are 5 steps, so
    # 30 x 6e-8 = 1.8e-6 of the buffer's largest magnitude bounds even errors that all add up
    tol = 2e-6 * float(want.abs().max())
    err = float((got.double() - want).abs().max())
    assert err <= tol, "{}: max error {} > {}".format(what, err, tol)


CASES = list(itertools.product([0.0, 0.9], [False, True], [0.0, 0.1], [0.0, 1e-2], sorted(CLIPS)))


@pytest.mark.parametrize("momentum,nesterov,decay,weight_decay,clip", CASES)
def test_torch_path_against_float64(momentum, nesterov, decay, weight_decay, clip):
    flat, gen = _flat()
    p0 = flat.data.clone()
    grads = _grads(flat, gen)
    opt = KerasSGD(flat, lr=LR, momentum=momentum, decay=decay, nesterov=nesterov, weight_decay=weight_decay,
                   clipnorm=CLIPS[clip], backend="torch")
    assert not opt._use_hip() and opt.class_name == "SGD"
    assert opt.segment_decay() == [weight_decay, 0.0, weight_decay]          # the rank-1 segment receives none
    for g in grads:
        flat.grad.copy_(g)
        opt.step()
    p, v, clipped = reference(flat, p0, grads, LR, momentum, nesterov, decay, weight_decay, CLIPS[clip])
    assert all(clipped) if clip == "active" else not any(clipped)
    assert opt.iterations == STEPS
    _close(flat.data, p, "p")
    _close(opt.velocity, v, "velocity")
    if weight_decay and not momentum and not nesterov and not decay:
        # decay moved the kernels and only them: against the same run without it
        q, _, _ = reference(flat, p0, grads, LR, momentum, nesterov, decay, 0.0, CLIPS[clip])
        s = flat.segments[1]
        assert torch.equal(p[s.offset:s.offset + s.numel], q[s.offset:s.offset + s.numel])
        assert not torch.equal(p, q)


def test_config_and_state():
    flat, _ = _flat()
    opt = KerasSGD(flat, lr=0.1, momentum=0.9, nesterov=True, decay=0.01, weight_decay=1e-4, clipnorm=2.0)
    assert opt.get_config() == {"lr": 0.1, "momentum": 0.9, "decay": 0.01, "nesterov": True, "clipnorm": 2.0,
                                "weight_decay": 1e-4}
    assert list(opt.state_tensors()) == ["velocity"] and opt.state_tensors()["velocity"] is opt.velocity
    assert opt.initial_lr == 0.1 and opt.base_lr(3) == pytest.approx(0.1 / 1.02)
    assert KerasAdam(flat).class_name == "Adam"
    with pytest.raises(ValueError):
        KerasSGD(flat, momentum=-0.1)


@pytest.mark.parametrize("clip_mode", ["local", "global"])
def test_through_distributed_optimizer(clip_mode):
    flat, gen = _flat(seed=3)
    p0 = flat.data.clone()
    grads = _grads(flat, gen)
    opt = KerasSGD(flat, lr=LR, momentum=0.9, weight_decay=1e-2, clipnorm=0.5, backend="torch")
    dist = DistributedOptimizer(opt, clip_mode=clip_mode)
    try:
        for g in grads:
            dist.zero_grad()
            flat.grad.copy_(g)
            norm = dist.step()
            assert float(norm) == pytest.approx(float(g.double().norm()), rel=1e-5)
    finally:
        dist.remove_hooks()
    p, v, clipped = reference(flat, p0, grads, LR, 0.9, False, 0.0, 1e-2, 0.5)
    assert all(clipped) and dist.iterations == STEPS
    _close(flat.data, p, "p")
    _close(dist.state_tensors()["velocity"], v, "velocity")


# ------------------------------------------------------------------------------------------------ checkpoints
def _trainer(optimizer, seed=0, **kw):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    torch.manual_seed(seed)
    model = models.backbone("resnet18").retinanet(3)
    return Trainer(model, lr=0.01, clipnorm=0.0, device=torch.device("cpu"), optimizer=optimizer, **kw)


def _fill_state(tr, seed):
    gen = torch.Generator().manual_seed(seed)
    flat = tr.flat
    for t in tr.base_optimizer.state_tensors().values():
        for s in flat.segments:      # the alignment padding between segments holds no state: a Keras file has none
            t[s.offset:s.offset + s.numel] = torch.randn(s.numel, generator=gen)
    tr.base_optimizer.iterations = 7


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_sgd_checkpoint_round_trip(tmp_path, ext):
    a = _trainer("sgd", seed=1, momentum=0.9, weight_decay=1e-4)
    _fill_state(a, 5)
    path = str(tmp_path / ("ck." + ext))
    checkpoint.save_checkpoint(path, a.model, a.base_optimizer, epoch=2)
    assert checkpoint.stored_optimizer_class(path) == "SGD"
    if ext == "h5":
        f = hdf5.File(path, "r")
        cfg = json.loads(bytes(f.attrs["training_config"]).decode())["optimizer_config"]
        assert cfg["class_name"] == "SGD" and cfg["config"]["momentum"] == 0.9 and cfg["config"]["weight_decay"] == 1e-4
        ow = f["optimizer_weights"]
        names = hdf5.load_attributes_from_hdf5_group(ow, "weight_names")
        params = checkpoint._keras_order_params(a.model)
        assert names[0] == "SGD/iterations:0" and names[1] == "training/SGD/Variable:0"
        assert names[2] == "training/SGD/Variable_1:0" and len(names) == 1 + len(params)
        assert int(np.asarray(ow[names[0]]).reshape(-1)[0]) == 7
        p, kind = params[0]                                              # a conv kernel: stored HWIO
        assert kind == "kernel" and np.asarray(ow[names[1]]).shape == tuple(p.shape[i] for i in (1, 2, 3, 0))
    b = _trainer("sgd", seed=2, momentum=0.9)
    assert not torch.equal(a.flat.data, b.flat.data)
    checkpoint.load_weights(b.model, path)
    assert checkpoint.load_optimizer(b.model, b.base_optimizer, path) is True
    b.on_weights_changed()
    assert torch.equal(a.flat.data, b.flat.data)
    assert torch.equal(a.base_optimizer.velocity, b.base_optimizer.velocity)
    assert b.base_optimizer.iterations == 7 and checkpoint.checkpoint_epoch(path) == 2


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_adam_snapshot_into_sgd_restores_weights_only(tmp_path, ext):
    a = _trainer("adam", seed=1)
    _fill_state(a, 6)
    path = str(tmp_path / ("adam." + ext))
    checkpoint.save_checkpoint(path, a.model, a.base_optimizer, epoch=1)
    assert checkpoint.stored_optimizer_class(path) == "Adam"
    b = _trainer("sgd", seed=2, momentum=0.9)
    checkpoint.load_weights(b.model, path)
    with pytest.warns(UserWarning, match="Adam.*SGD"):
        assert checkpoint.load_optimizer(b.model, b.base_optimizer, path) is False
    b.on_weights_changed()
    assert torch.equal(a.flat.data, b.flat.data)
    assert not b.base_optimizer.velocity.any() and b.base_optimizer.iterations == 0
    # and the other way round
    c = _trainer("adam", seed=3)
    spath = str(tmp_path / ("sgd." + ext))
    _fill_state(b, 8)
    checkpoint.save_checkpoint(spath, b.model, b.base_optimizer)
    with pytest.warns(UserWarning, match="SGD.*Adam"):
        assert checkpoint.load_optimizer(c.model, c.base_optimizer, spath) is False
    assert not c.base_optimizer.m.any() and not c.base_optimizer.v.any() and c.base_optimizer.iterations == 0


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_adam_files_are_unchanged(tmp_path, ext):
    """An Adam checkpoint says what it said before SGD existed: the same bytes from a trainer built without the
    new arguments and from one that names ``optimizer='adam'``, class name Adam, slots m and v."""
    a = _trainer("adam", seed=4)
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    from batchai_retinanet_horovod_coco_amd import models
    torch.manual_seed(4)
    b = Trainer(models.backbone("resnet18").retinanet(3), lr=0.01, clipnorm=0.0, device=torch.device("cpu"))
    for tr in (a, b):
        _fill_state(tr, 9)
    pa, pb = str(tmp_path / ("a." + ext)), str(tmp_path / ("b." + ext))
    checkpoint.save_checkpoint(pa, a.model, a.base_optimizer, epoch=3)
    checkpoint.save_checkpoint(pb, b.model, b.base_optimizer, epoch=3)
    ra, rb = open(pa, "rb").read(), open(pb, "rb").read()
    if ext == "h5":
        assert ra == rb
    else:
        # the safetensors writer lays its metadata map out in an order that varies from one save to the next: the
        # header is compared as the JSON it is, the tensor bytes behind it as bytes
        na, nb = (int.from_bytes(r[:8], "little") for r in (ra, rb))
        assert json.loads(ra[8:8 + na]) == json.loads(rb[8:8 + nb]) and ra[8 + na:] == rb[8 + nb:]
    assert checkpoint.training_config(a.base_optimizer)["optimizer_config"] == {
        "class_name": "Adam", "config": a.base_optimizer.get_config()}
    if ext == "h5":
        names = hdf5.load_attributes_from_hdf5_group(hdf5.File(pa, "r")["optimizer_weights"], "weight_names")
        n = len(checkpoint._keras_order_params(a.model))
        assert names[0] == "Adam/iterations:0" and len(names) == 1 + 3 * n
    else:
        from safetensors import safe_open
        with safe_open(pa, framework="pt") as f:
            assert {"__optimizer__.m", "__optimizer__.v"} <= set(f.keys()) and "__optimizer__.velocity" not in f.keys()
            assert set(f.metadata()) == {"model_config", "framework", "epoch", "iterations", "lr", "training_config"}


# ------------------------------------------------------------------------------------------------ CLI
def test_flags_parse():
    a = T.parse_args(["coco", "/x"])
    assert a.optimizer == "adam" and a.momentum == 0.9 and not a.nesterov and a.weight_decay == 0 and a.warmup_epochs == 0
    assert a.lr == 1e-5 and a.clipnorm == 0.001
    a = T.parse_args(["--optimizer", "sgd", "--momentum", "0.8", "--nesterov", "--weight-decay", "1e-4",
                      "--warmup-epochs", "3", "--lr", "0.08", "--clipnorm", "0", "coco", "/x"])
    assert (a.optimizer, a.momentum, a.nesterov, a.weight_decay, a.warmup_epochs) == ("sgd", 0.8, True, 1e-4, 3)
    assert "SGD" in T.build_parser().format_help().replace("\n", " ")


def test_weight_decay_with_adam_exits():
    with pytest.raises(SystemExit, match="weight-decay"):
        T.parse_args(["--weight-decay", "1e-4", "coco", "/x"])
    with pytest.raises(SystemExit, match="weight-decay"):
        T.parse_args(["--optimizer", "adam", "--weight-decay", "1e-4", "coco", "/x"])


def test_optimizer_flag_against_snapshot(tmp_path):
    a = _trainer("sgd", momentum=0.9)
    path = str(tmp_path / "sgd.h5")
    checkpoint.save_checkpoint(path, a.model, a.base_optimizer, epoch=1)
    with pytest.raises(SystemExit, match="adam.*sgd"):
        T.parse_args(["--snapshot", path, "--optimizer", "adam", "coco", "/x"])
    assert T.parse_args(["--snapshot", path, "coco", "/x"]).optimizer == "sgd"       # the file decides
    assert T.parse_args(["--snapshot", path, "--optimizer", "sgd", "--weight-decay", "1e-4", "coco", "/x"]).optimizer == "sgd"


def test_cli_sgd_warmup_checkpoint_resume(tmp_path):
    common = ["--no-weights", "--backbone", "resnet18", "--batch-size", "2", "--image-min-side", "64",
              "--image-max-side", "96", "--snapshot-path", str(tmp_path / "snap"), "--tensorboard-dir", "",
              "--device", "cpu", "--workers", "1", "--seed", "1", "--no-evaluation"]
    data = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "4", "--max-boxes", "3"]
    h = T.main(common + ["--optimizer", "sgd", "--momentum", "0.9", "--warmup-epochs", "1", "--epochs", "2",
                         "--steps", "2", "--lr", "1e-3"] + data)
    assert len(h.history["loss"]) == 2 and all(v == v for v in h.history["loss"])
    ck = str(tmp_path / "snap" / "checkpoint-02.h5")
    assert os.path.exists(ck) and checkpoint.stored_optimizer_class(ck) == "SGD"
    f = hdf5.File(ck, "r")
    assert int(np.asarray(f["optimizer_weights/SGD/iterations:0"]).reshape(-1)[0]) == 4
    # resume: no --optimizer, the snapshot says SGD; iterations continue
    h2 = T.main(["--snapshot", ck] + common[1:] + ["--epochs", "3", "--steps", "1", "--lr", "1e-3"] + data)
    assert h2.epoch == [2]
    f = hdf5.File(str(tmp_path / "snap" / "checkpoint-03.h5"), "r")
    assert int(np.asarray(f["optimizer_weights/SGD/iterations:0"]).reshape(-1)[0]) == 5
    assert glob.glob(str(tmp_path / "snap" / "checkpoint-0*.h5"))


# ------------------------------------------------------------------------------------------------ momentum correction
class _Stub:
    def __init__(self, lr, momentum=None):
        self.lr = lr
        if momentum is not None:
            self.momentum = momentum


def test_momentum_correction_for_one_step():
    m = _Stub(lr=0.1, momentum=0.9)
    cb = hvd_callbacks.LearningRateScheduleCallback(multiplier=2.0, initial_lr=0.1)      # a step that doubles lr
    cb.set_model(m)
    cb.on_train_begin()
    cb.on_epoch_begin(0)
    assert m.lr == pytest.approx(0.2) and m.momentum == pytest.approx(1.8)
    cb.on_batch_begin(0)
    cb.on_batch_end(0)
    assert m.momentum == 0.9 and m.lr == pytest.approx(0.2)
    cb.on_batch_begin(1)
    assert m.momentum == 0.9
    cb.on_batch_end(1)
    assert m.momentum == 0.9


def test_warmup_momentum_correction(monkeypatch):
    from batchai_retinanet_horovod_coco_amd.parallel import runtime
    monkeypatch.setattr(runtime, "is_initialized", lambda: True)
    monkeypatch.setattr(runtime, "size", lambda: 3)
    m = _Stub(lr=0.3, momentum=0.9)
    cb = hvd_callbacks.LearningRateWarmupCallback(warmup_epochs=1, steps_per_epoch=2)
    cb.set_model(m)
    cb.on_train_begin()
    cb.on_epoch_begin(0)
    cb.on_batch_begin(0)                      # lr 0.3 -> 0.1
    assert m.lr == pytest.approx(0.1) and m.momentum == pytest.approx(0.3)
    cb.on_batch_end(0)
    assert m.momentum == 0.9
    cb.on_batch_begin(1)                      # 0.1 -> 0.2: this step runs at 2 x momentum
    assert m.lr == pytest.approx(0.2) and m.momentum == pytest.approx(1.8)
    cb.on_batch_end(1)
    assert m.momentum == 0.9
    off = hvd_callbacks.LearningRateWarmupCallback(warmup_epochs=1, steps_per_epoch=2, momentum_correction=False)
    n = _Stub(lr=0.3, momentum=0.9)
    off.set_model(n)
    off.on_train_begin()
    off.on_batch_begin(0)
    assert n.lr == pytest.approx(0.1) and n.momentum == 0.9


def test_model_without_momentum_is_left_alone():
    m = _Stub(lr=0.1)
    cb = hvd_callbacks.LearningRateScheduleCallback(multiplier=2.0, initial_lr=0.1)
    cb.set_model(m)
    cb.on_train_begin()
    cb.on_epoch_begin(0)
    cb.on_batch_end(0)
    assert m.lr == pytest.approx(0.2) and not hasattr(m, "momentum")
    tr = _trainer("adam")
    assert not hasattr(tr, "momentum")
    cb.set_model(tr)
    cb.on_epoch_begin(0)
    cb.on_batch_end(0)
    assert tr.lr == pytest.approx(0.2)
    sgd = _trainer("sgd", momentum=0.9)
    sgd.momentum = 0.5
    assert sgd.momentum == 0.5 and sgd.base_optimizer.momentum == 0.5
