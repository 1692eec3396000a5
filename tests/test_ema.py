"""The weight EMA carried by the optimizer step (``ema_decay``), on the CPU: the torch expression of both optimizers
against float64 with the fp32 decay ramp ``d_n = min(D, (1 + n) / (10 + n))`` checked exactly; off means off;
checkpoints of both formats with the ``ema_weights`` group / ``ema/`` tensors and the mixed cases;
``Trainer.ema_weights()``; the ``EmaWeights`` evaluation callback; the ``train.py`` flags; and a gloo world of two in
which the broadcast carries the average and its update count."""
import os
import socket
import tempfile
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.io import checkpoint, hdf5
from batchai_retinanet_horovod_coco_amd.train.flat import FlatParams
from batchai_retinanet_horovod_coco_amd.train.optimizer import KerasAdam, KerasSGD

# the segments of tests/test_sgd_gpu.py
SHAPES = [(7, 3, 3, 5), (13,), (64, 1, 1, 64), (3, 8195), (2, 8192)]
SENTINEL = -12345.0


def ramp(D, n):
    """d_n as the issue states it: fp32 division, then min with fp32(D)."""
    return float(min(np.float32(D), np.float32(1 + n) / np.float32(10 + n)))


def _flat(seed=0):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SHAPES]
    flat = FlatParams([(str(i), p) for i, p in enumerate(params)])
    pad = torch.ones(flat.total, dtype=torch.bool)
    for s in flat.segments:
        pad[s.offset:s.offset + s.numel] = False
    return flat, gen, pad


def _grad(flat, gen, pad):
    g = torch.randn(flat.total, generator=gen)
    g[pad] = 0
    return g


def _bound_ok(got, want, pad, what):
    """The project's per-element bound: 1e-5 |ref| + 1e-6 max |ref|."""
    real = ~pad
    got, want = got[real].double(), want[real].double()
    bound = 1e-5 * want.abs() + 1e-6 * float(want.abs().max())
    err = (got - want).abs()
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


# ------------------------------------------------------------------------------------------------ the ramp
def test_decay_ramp_is_exact_fp32():
    flat, _, _ = _flat()
    opt = KerasSGD(flat, backend="torch", ema_decay=0.5)
    seq = [opt.ema_decay_at(n) for n in range(1, 13)]
    assert seq == [ramp(0.5, n) for n in range(1, 13)]
    assert seq[0] == float(np.float32(2) / np.float32(11))
    assert all(a < b for a, b in zip(seq[:7], seq[1:8]))        # the ramp rises ...
    assert seq[6] < 0.5 and seq[7:] == [0.5] * 5                # ... and reaches the cap at n = 8 (9 / 18)
    pure = KerasAdam(flat, backend="torch", ema_decay=0.9999)
    assert all(pure.ema_decay_at(n) == float(np.float32(1 + n) / np.float32(10 + n)) < 0.9999 for n in range(1, 13))
    assert pure.ema_decay_at(10 ** 6) == float(np.float32(0.9999))
    with pytest.raises(ValueError):
        KerasAdam(flat, backend="torch", ema_decay=1.0)
    with pytest.raises(ValueError):
        KerasSGD(flat, backend="torch", ema_decay=-0.1)


# ------------------------------------------------------------------------------------------------ torch backend
@pytest.mark.parametrize("D", [0.5, 0.9999])
@pytest.mark.parametrize("which", ["adam", "sgd_momentum"])
def test_torch_backend_against_float64(which, D):
    flat, gen, pad = _flat(3)
    flat.data[pad] = SENTINEL
    if which == "adam":
        opt = KerasAdam(flat, lr=1e-3, clipnorm=0.5, backend="torch", ema_decay=D)
        m64 = torch.zeros(flat.total, dtype=torch.float64)
        v64 = torch.zeros_like(m64)
    else:
        opt = KerasSGD(flat, lr=1e-2, momentum=0.9, clipnorm=0.5, backend="torch", ema_decay=D)
        v64 = torch.zeros(flat.total, dtype=torch.float64)
    assert opt.ema is not None and opt.ema.dtype == torch.float32 and opt.ema.shape == flat.data.shape
    assert torch.equal(opt.ema, flat.data) and opt.ema.data_ptr() != flat.data.data_ptr()       # seeded with a copy
    p64 = flat.data.double()
    full64 = p64.clone()            # the average of the float64 run
    iso64 = p64.clone()             # the average over the backend's own weights: the EMA arithmetic alone
    for n in range(1, 13):
        g = _grad(flat, gen, pad)
        flat.grad.copy_(g)
        norm, factor = opt.norm_and_scale()
        opt.step()
        f, g = float(factor), g.double()
        if which == "adam":
            b1, b2 = opt.beta_1, opt.beta_2
            m64 = b1 * m64 + (1 - b1) * g * f
            v64 = b2 * v64 + (1 - b2) * (g * f) ** 2
            p64 = p64 - opt.lr_t(n) * m64 / (v64.sqrt() + opt.epsilon)
        else:
            v64 = 0.9 * v64 - 1e-2 * g * f
            p64 = p64 + v64
        d = ramp(D, n)
        assert opt.ema_updates == n and opt.ema_decay_at(n) == d
        full64 = d * full64 + (1 - d) * p64
        iso64 = d * iso64 + (1 - d) * flat.data.double()
        _bound_ok(opt.ema, iso64, pad, ("ema, own weights", n))
        _bound_ok(opt.ema, full64, pad, ("ema, float64 run", n))
        _bound_ok(flat.data, p64, pad, ("p", n))
    assert bool((flat.data[pad] == SENTINEL).all())
    assert opt.iterations == 12 and opt.ema_start == 0
    assert set(opt.state_tensors()) == ({"m", "v", "ema"} if which == "adam" else {"velocity", "ema"})
    assert opt.get_config()["ema_decay"] == D


@pytest.mark.parametrize("which", ["adam", "sgd"])
def test_off_means_off(which):
    def run(**kw):
        flat, gen, pad = _flat(5)
        opt = (KerasAdam(flat, lr=1e-3, backend="torch", **kw) if which == "adam" else
               KerasSGD(flat, lr=1e-2, momentum=0.9, backend="torch", **kw))
        for _ in range(5):
            flat.grad.copy_(_grad(flat, gen, pad))
            opt.step()
        return flat.data.clone(), opt
    p0, a = run()
    p1, b = run(ema_decay=0.0)
    assert torch.equal(p0, p1)
    assert a.state_tensors().keys() == b.state_tensors().keys() and "ema" not in b.state_tensors()
    for k in a.state_tensors():
        assert torch.equal(a.state_tensors()[k], b.state_tensors()[k])
    assert b.ema is None and a.get_config() == b.get_config() and "ema_decay" not in b.get_config()
    assert checkpoint.training_config(a) == checkpoint.training_config(b)
    # and with the average on, the weights and slots are the same: it only reads them
    p2, c = run(ema_decay=0.5)
    assert torch.equal(p0, p2) and c.ema is not None and not torch.equal(c.ema, p2)


# ------------------------------------------------------------------------------------------------ trainers
def _trainer(optimizer="adam", seed=0, **kw):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    torch.manual_seed(seed)
    model = models.backbone("resnet18").retinanet(3)
    if optimizer == "sgd":
        kw = dict(kw, optimizer="sgd", momentum=0.9)
    return Trainer(model, lr=1e-3, clipnorm=10.0, device=torch.device("cpu"), **kw)


def _batches(n, seed=7):
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    g = torch.Generator().manual_seed(seed)
    return [make_batch(1, 64, 96, num_classes=3, max_boxes=3, generator=g) for _ in range(n)]


def _train(tr, batches):
    for b in batches:
        tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])


def _state(tr):
    opt = tr.base_optimizer
    return dict(opt.state_tensors(), p=tr.flat.data)


@pytest.fixture(scope="module")
def six_steps(tmp_path_factory):
    """Per optimizer: the state after 6 uninterrupted steps, and snapshots of both formats taken after step 3."""
    out = {}
    d = tmp_path_factory.mktemp("ema")
    batches = _batches(6)
    for which, ext in (("adam", "h5"), ("sgd", "safetensors")):
        tr = _trainer(which, seed=1, ema_decay=0.5)
        _train(tr, batches[:3])
        path = str(d / "{}.{}".format(which, ext))
        checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
        mid = {k: v.clone() for k, v in _state(tr).items()}
        _train(tr, batches[3:])
        out[which] = (path, mid, {k: v.clone() for k, v in _state(tr).items()}, tr.base_optimizer.ema_updates)
    return batches, out


@pytest.mark.parametrize("which", ["adam", "sgd"])
def test_checkpoint_round_trip(six_steps, which):
    batches, runs = six_steps
    path, mid, end, updates = runs[which]
    assert updates == 6 and checkpoint.has_ema_weights(path)
    if path.endswith(".h5"):
        g = hdf5.File(path, "r")["ema_weights"]
        assert float(np.asarray(g.attrs["ema_decay"]).reshape(-1)[0]) == 0.5
        assert int(np.asarray(g.attrs["ema_updates"]).reshape(-1)[0]) == 3
        mw = hdf5.File(path, "r")["model_weights"]
        assert hdf5.load_attributes_from_hdf5_group(g, "layer_names") == \
            hdf5.load_attributes_from_hdf5_group(mw, "layer_names")
    else:
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            meta = f.metadata()
            assert meta["ema_decay"] == "0.5" and meta["ema_updates"] == "3"
            assert {"ema/" + k for k in f.keys() if not k.startswith(("ema/", "__optimizer__."))} == \
                {k for k in f.keys() if k.startswith("ema/")}
    tr = _trainer(which, seed=2, ema_decay=0.5)
    assert not torch.equal(tr.flat.data, mid["p"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert checkpoint.restore_checkpoint(path, tr.model, tr.base_optimizer) == 1
    tr.on_weights_changed()
    assert tr.base_optimizer.ema_updates == 3 and tr.base_optimizer.iterations == 3
    for k, v in _state(tr).items():
        assert torch.equal(v, mid[k]), k
    _train(tr, batches[3:])
    assert tr.base_optimizer.ema_updates == 6
    for k, v in _state(tr).items():
        assert torch.equal(v, end[k]), k
    assert not torch.equal(end["ema"], end["p"])


@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_mixed_snapshots(six_steps, tmp_path, ext):
    batches, runs = six_steps
    # a file written with the EMA off: no averaged set, and nothing new in it
    off = _trainer("adam", seed=1)
    _train(off, batches[:1])
    plain = str(tmp_path / ("plain." + ext))
    checkpoint.save_checkpoint(plain, off.model, off.base_optimizer, epoch=1)
    assert not checkpoint.has_ema_weights(plain)
    if ext == "h5":
        assert set(hdf5.File(plain, "r").keys()) == {"model_weights", "optimizer_weights"}
    else:
        from safetensors import safe_open
        with safe_open(plain, framework="pt") as f:
            assert not any(k.startswith("ema") for k in f.keys())
            assert set(f.metadata()) == {"model_config", "framework", "epoch", "iterations", "lr", "training_config"}
    # ... loaded into an EMA run: the average is seeded from the weights, with one warning
    on = _trainer("adam", seed=2, ema_decay=0.5)
    with pytest.warns(UserWarning, match="ema_weights") as rec:
        checkpoint.restore_checkpoint(plain, on.model, on.base_optimizer)
    assert len([w for w in rec if "ema_weights" in str(w.message)]) == 1
    on.on_weights_changed()
    assert on.base_optimizer.iterations == 1 and on.base_optimizer.ema_updates == 0
    assert torch.equal(on.base_optimizer.ema, on.flat.data) and torch.equal(on.flat.data, off.flat.data)
    with pytest.raises(ValueError):
        checkpoint.load_weights(on.model, plain, group="ema_weights")
    with pytest.raises(SystemExit, match="weights-ema"):
        T.parse_args(["--weights", plain, "--weights-ema", "coco", "/x"])
    # a file with the averaged set loaded into a run without one: ignored
    which = "adam" if ext == "h5" else "sgd"
    path, mid, _, _ = runs[which]
    no = _trainer(which, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        checkpoint.restore_checkpoint(path, no.model, no.base_optimizer)
    no.on_weights_changed()
    assert no.base_optimizer.ema is None and torch.equal(no.flat.data, mid["p"])
    assert no.base_optimizer.iterations == 3
    # the averaged set as a weight set: trainable tensors hold the average, the others what model_weights hold
    from batchai_retinanet_horovod_coco_amd import models
    m = models.backbone("resnet18").retinanet(3)
    checkpoint.load_weights(m, path, group="ema_weights")
    got = FlatParams([(n, p) for n, p in reversed([(n, p) for n, p in m.named_parameters() if p.requires_grad])])
    assert torch.equal(got.data, mid["ema"]) and not torch.equal(got.data, mid["p"])
    for (k, a), (_, b) in zip(m.state_dict().items(), no.model.state_dict().items()):
        if k not in dict(m.named_parameters()) or not dict(m.named_parameters())[k].requires_grad:
            assert torch.equal(a, b), k
    assert T.parse_args(["--weights", path, "--weights-ema", "coco", "/x"]).weights_ema


def test_context_manager():
    tr = _trainer("sgd", seed=4, ema_decay=0.5)
    _train(tr, _batches(2))
    p, e = tr.flat.data.clone(), tr.base_optimizer.ema.clone()
    ptr = tr.flat.data.data_ptr()
    assert not torch.equal(p, e)
    with tr.ema_weights():
        assert torch.equal(tr.flat.data, e) and torch.equal(tr.base_optimizer.ema, p)
        assert tr.flat.data.data_ptr() == ptr
        first = next(iter(tr.flat.segments))
        assert torch.equal(first.param.data.reshape(-1), e[first.offset:first.offset + first.numel])
        with pytest.raises(RuntimeError, match="already inside"):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            _train(tr, _batches(1))
    assert torch.equal(tr.flat.data, p) and torch.equal(tr.base_optimizer.ema, e)
    # an exception inside still exchanges back
    with pytest.raises(KeyError):
        with tr.ema_weights():
            raise KeyError("x")
    assert torch.equal(tr.flat.data, p) and torch.equal(tr.base_optimizer.ema, e)
    with tr.ema_weights():          # and it can be entered again
        pass
    with pytest.raises(RuntimeError, match="no weight EMA"):
        with _trainer("adam", seed=4).ema_weights():
            pass


def test_reseed_only_before_the_first_update():
    tr = _trainer("adam", seed=5, ema_decay=0.5)
    with torch.no_grad():
        tr.flat.data.mul_(2.0)      # weights replaced before any step (--weights, broadcast)
    tr.on_weights_changed()
    assert torch.equal(tr.base_optimizer.ema, tr.flat.data)
    _train(tr, _batches(1))
    e = tr.base_optimizer.ema.clone()
    tr.on_weights_changed()
    assert torch.equal(tr.base_optimizer.ema, e) and tr.base_optimizer.ema_updates == 1


def test_evaluation_callback_sees_the_average():
    from batchai_retinanet_horovod_coco_amd.train import callbacks as kc
    tr = _trainer("adam", seed=6, ema_decay=0.5)
    _train(tr, _batches(2))
    p, e = tr.flat.data.clone(), tr.base_optimizer.ema.clone()
    seen = {}

    class Stub(kc.Callback):
        def on_train_begin(self, logs=None):
            seen["begin"] = tr.flat.data.clone()

        def on_epoch_end(self, epoch, logs=None):
            seen["epoch"] = epoch
            seen["w"] = self.model.regression_submodel.convs()[0].weight.detach().clone()
            seen["flat"] = tr.flat.data.clone()
            logs["mAP"] = 0.25

    cb = kc.EmaWeights(kc.RedirectModel(Stub(), tr.model), tr)
    cb.set_model(tr)
    cb.set_params({"epochs": 1})
    cb.on_train_begin({})
    logs = {}
    cb.on_epoch_end(3, logs)
    assert torch.equal(seen["begin"], p)                    # only the epoch's end runs on the average
    assert seen["epoch"] == 3 and logs == {"mAP": 0.25}
    assert torch.equal(seen["flat"], e)
    seg = tr.flat.by_param[id(tr.model.regression_submodel.convs()[0].weight)]
    assert torch.equal(seen["w"].reshape(-1), e[seg.offset:seg.offset + seg.numel])
    assert torch.equal(tr.flat.data, p) and torch.equal(tr.base_optimizer.ema, e)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_flags():
    a = T.parse_args(["coco", "/x"])
    assert a.ema_decay == 0.0 and a.weights_ema is False
    assert T.parse_args(["--ema-decay", "0.9998", "coco", "/x"]).ema_decay == 0.9998
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit, match="ema-decay"):
            T.parse_args(["--ema-decay=" + bad, "coco", "/x"])
    with pytest.raises(SystemExit, match="weights-ema"):
        T.parse_args(["--weights-ema", "coco", "/x"])


def test_cli_trains_evaluates_snapshots_resumes(tmp_path):
    common = ["--no-weights", "--backbone", "resnet18", "--batch-size", "1", "--image-min-side", "64",
              "--image-max-side", "96", "--snapshot-path", str(tmp_path / "snap"), "--tensorboard-dir", "",
              "--device", "cpu", "--workers", "1", "--seed", "1", "--ema-decay", "0.9998"]
    data = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "3", "--max-boxes", "3"]
    h = T.main(common + ["--epochs", "2", "--steps", "2", "--lr", "1e-3"] + data)
    assert len(h.history["loss"]) == 2 and "mAP" in h.history
    ck = str(tmp_path / "snap" / "checkpoint-02.h5")
    g = hdf5.File(ck, "r")["ema_weights"]
    assert int(np.asarray(g.attrs["ema_updates"]).reshape(-1)[0]) == 4
    assert float(np.asarray(g.attrs["ema_decay"]).reshape(-1)[0]) == 0.9998
    h2 = T.main(["--snapshot", ck] + common[1:] + ["--epochs", "3", "--steps", "1", "--lr", "1e-3"] + data)
    assert h2.epoch == [2]
    g = hdf5.File(str(tmp_path / "snap" / "checkpoint-03.h5"), "r")["ema_weights"]
    assert int(np.asarray(g.attrs["ema_updates"]).reshape(-1)[0]) == 5


# ------------------------------------------------------------------------------------------------ gloo, world 2
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _w_broadcast(rank, world, port, out):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "LOCAL_WORLD_SIZE": str(world)})
    from batchai_retinanet_horovod_coco_amd.parallel import runtime
    runtime.init(backend="gloo", device="cpu", timeout_s=60)
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    from batchai_retinanet_horovod_coco_amd.parallel.callbacks import BroadcastGlobalVariablesCallback
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    torch.manual_seed(100 + rank)
    tr = Trainer(models.backbone("resnet18").retinanet(3), lr=1e-4, clip_mode="global", device=torch.device("cpu"),
                 ema_decay=0.5)
    opt = tr.base_optimizer
    # rank 0 as a restore leaves it: 7 steps done, 3 of them averaged; rank 1 somewhere else entirely
    opt.iterations, opt.ema_start = (7, 4) if rank == 0 else (2, 1)
    with torch.no_grad():
        opt.ema.add_(0.25 * (rank + 1))
    before = opt.ema.clone()
    cb = BroadcastGlobalVariablesCallback(0)
    cb.set_model(tr)
    cb.on_train_begin()
    after_bcast = (opt.iterations, opt.ema_start, opt.ema.clone())
    g = torch.Generator().manual_seed(rank)
    for _ in range(2):
        b = make_batch(1, 64, 96, num_classes=3, max_boxes=3, generator=g)
        tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    torch.save({"ema": opt.ema.clone(), "w": tr.flat.data.clone(), "updates": opt.ema_updates, "it": opt.iterations,
                "start": opt.ema_start, "before": before, "bcast": after_bcast},
               os.path.join(out, "r{}.pt".format(rank)))
    runtime.shutdown()


def test_broadcast_carries_the_average_world2():
    out = tempfile.mkdtemp()
    mp.spawn(_w_broadcast, args=(2, _port(), out), nprocs=2, join=True)
    r0 = torch.load(os.path.join(out, "r0.pt"), weights_only=False)
    r1 = torch.load(os.path.join(out, "r1.pt"), weights_only=False)
    assert not torch.equal(r0["before"], r1["before"])
    assert r1["bcast"][:2] == (7, 4) and torch.equal(r1["bcast"][2], r0["before"])       # rank 0's, not re-seeded
    assert torch.equal(r0["bcast"][2], r0["before"])
    assert r0["updates"] == r1["updates"] == 5 and r0["it"] == r1["it"] == 9 and r0["start"] == r1["start"] == 4
    assert torch.equal(r0["w"], r1["w"]) and torch.equal(r0["ema"], r1["ema"])
    assert not torch.equal(r0["ema"], r0["w"])
