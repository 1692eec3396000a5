"""``Trainer(ema_decay=0.5)`` through captured steps (``Trainer.enable_graphs``) is BIT-identical to the eager run, with
both optimizers: the decay of every replayed EMA update comes from the device step counter (the one-thread prologue
writes ``hyper[3]``), so it differs at each of the six replays -- a decay frozen at its capture-time value ends
elsewhere.  Midway a hook evaluates inside ``Trainer.ema_weights()``: the exchange moves no pointer, so nothing is
invalidated and the two runs stay identical; and the forward it runs equals, bit for bit, the forward of a second
trainer whose model loaded the averaged set (``group="ema_weights"``) from a snapshot written at that step, which ties
the exchange, the rebuilt compute copies (flipped and hx32-packed) and the file group together."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 8
BOXES = [3, 7, 5, 4, 3, 7, 5, 4]
OPTIMIZERS = {"sgd": dict(optimizer="sgd", momentum=0.9, weight_decay=1e-4), "adam": {}}


@pytest.fixture(scope="module")
def setup(cuda):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in models.backbone("resnet18").retinanet(8).state_dict().items()}
    g = torch.Generator().manual_seed(12)
    batches = [{k: v.to(cuda) for k, v in make_batch(1, 128, 192, num_classes=8, max_boxes=n, generator=g).items()}
               for n in BOXES]
    _run(cuda, state, batches[:1], None, "sgd")      # first sight: the conv tuner races here
    return state, batches


def _trainer(cuda, model, which, **kw):
    from batchai_retinanet_horovod_coco_amd.ops import native
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    native.set_grad_sinks(None)
    native.set_compute_weights(None)
    return Trainer(model, lr=1e-3, clipnorm=10.0, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda,
                   **dict(OPTIMIZERS[which], **kw))


def _forward(tr, images):
    """The raw outputs of the network the prediction model wraps."""
    with torch.no_grad():
        out = tr.model(images.to(torch.bfloat16))
    return out["regression"].clone(), out["classification"].clone()


def _run(cuda, state, batches, graphs, which, hook=None):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native
    model = models.backbone("resnet18").retinanet(8)
    model.load_state_dict(state)
    tr = _trainer(cuda, model, which, ema_decay=0.5)
    try:
        opt = tr.base_optimizer
        assert opt.ema is not None and tr.adam_plan() is not None
        if graphs is not None:
            tr.enable_graphs(**graphs)
        losses = []
        for i, b in enumerate(batches):
            if hook is not None:
                hook(i, tr)
            logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            losses.append(logs["loss"].clone())
        torch.cuda.synchronize()
        plan = tr.adam_plan()
        assert plan.iter.item() == plan.host_iter == opt.iterations == len(batches)
        stats = tr.step_graphs.stats() if tr.step_graphs is not None else None
        slots = {k: v.clone() for k, v in opt.state_tensors().items()}
        return {"loss": torch.stack(losses), "weights": tr.flat.data.clone(), "slots": slots,
                "iterations": opt.iterations, "stats": stats}
    finally:
        if tr.step_graphs is not None:
            tr.step_graphs.invalidate()
        native.set_grad_sinks(None)
        native.set_compute_weights(None)


def _same(a, b):
    assert a["iterations"] == b["iterations"]
    for name in ("loss", "weights"):
        assert torch.equal(a[name], b[name]), (name, (a[name].float() - b[name].float()).abs().max().item())
    assert a["slots"].keys() == b["slots"].keys() and "ema" in a["slots"]
    for k in a["slots"]:
        assert torch.equal(a["slots"][k], b["slots"][k]), (k, (a["slots"][k] - b["slots"][k]).abs().max().item())


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_replays_equal_the_eager_run(cuda, setup, tmp_path, which):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.io import checkpoint
    from batchai_retinanet_horovod_coco_amd.ops import native
    state, batches = setup
    seen = {}

    def evaluate(name, path=None):
        def hook(i, tr):
            if i != 5:
                return
            if path is not None:
                checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
            before = tr.flat.data.clone()
            with tr.ema_weights():
                assert not torch.equal(tr.flat.data, before)
                seen[name] = _forward(tr, batches[0]["images"])
            assert torch.equal(tr.flat.data, before)
        return hook

    snap = str(tmp_path / "step5.h5")
    eager = _run(cuda, state, batches, None, which, evaluate("eager", snap))
    graph = _run(cuda, state, batches, dict(eager_sightings=2), which, evaluate("graph"))
    st = graph["stats"]
    print(st)
    # one class, captured once, never invalidated: the exchange inside ema_weights() moved no pointer
    assert len(st["captured_classes"]) == 1 and st["captures"] == 1 and st["eager_only"] == {}
    assert st["invalidations"] == 0
    assert st["eager_steps"] == 2 and st["replayed_steps"] == STEPS - 2
    assert eager["iterations"] == graph["iterations"] == STEPS
    assert bool(torch.isfinite(eager["loss"]).all())
    _same(eager, graph)
    for a, b in zip(seen["eager"], seen["graph"]):
        assert torch.equal(a, b)
    assert not torch.equal(eager["slots"]["ema"], eager["weights"])

    # a decay frozen at the capture (the third step: d_3) cannot pass: held there, the average ends elsewhere
    def frozen(i, tr):
        if i >= 3:
            tr.base_optimizer.ema_start = i - 2         # n = iterations + 1 - ema_start stays 3
    held = _run(cuda, state, batches, None, which, frozen)
    assert torch.equal(held["weights"], graph["weights"])                   # the same weights ...
    assert not torch.equal(held["slots"]["ema"], graph["slots"]["ema"])     # ... another average

    # the forward inside the context against a second trainer on the snapshot's averaged set
    model2 = models.backbone("resnet18").retinanet(8)
    checkpoint.load_weights(model2, snap, group="ema_weights")
    tr2 = _trainer(cuda, model2, which)
    try:
        assert tr2.base_optimizer.ema is None and tr2.compute_weights is not None
        reg, cls = _forward(tr2, batches[0]["images"])
    finally:
        native.set_grad_sinks(None)
        native.set_compute_weights(None)
    assert torch.equal(reg, seen["eager"][0]) and torch.equal(cls, seen["eager"][1])
    assert bool(torch.isfinite(reg.float()).all()) and bool(cls.float().abs().sum() > 0)
