"""``Trainer(optimizer="sgd")`` through captured steps (``Trainer.enable_graphs``) is BIT-identical to the eager run:
one shape class, the learning rate lowered and the momentum changed for a single step after replays have begun -- both
are written outside the graph (``AdamPlan.set_lr`` / ``set_momentum``) and read from device memory by the replayed
fused SGD kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 8
BOXES = [3, 7, 5, 4, 3, 7, 5, 4]


@pytest.fixture(scope="module")
def setup(cuda):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in models.backbone("resnet18").retinanet(8).state_dict().items()}
    g = torch.Generator().manual_seed(12)
    batches = [{k: v.to(cuda) for k, v in make_batch(1, 128, 192, num_classes=8, max_boxes=n, generator=g).items()}
               for n in BOXES]
    _run(cuda, state, batches[:1], None)      # first sight: the conv tuner races here
    return state, batches


def _run(cuda, state, batches, graphs, hook=None):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    native.set_grad_sinks(None)
    native.set_compute_weights(None)
    model = models.backbone("resnet18").retinanet(8)
    model.load_state_dict(state)
    tr = Trainer(model, lr=1e-3, clipnorm=10.0, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda,
                 optimizer="sgd", momentum=0.9, weight_decay=1e-4)
    try:
        assert tr.base_optimizer.class_name == "SGD" and tr.adam_plan() is not None
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
        assert plan.iter.item() == plan.host_iter == tr.base_optimizer.iterations
        stats = tr.step_graphs.stats() if tr.step_graphs is not None else None
        return (torch.stack(losses), tr.flat.data.clone(), tr.base_optimizer.velocity.clone(),
                tr.base_optimizer.iterations, stats)
    finally:
        if tr.step_graphs is not None:
            tr.step_graphs.invalidate()
        native.set_grad_sinks(None)
        native.set_compute_weights(None)


def _hook(i, tr):
    if i == 5:
        tr.lr *= 0.1            # what ReduceLROnPlateau does; replays began at step 2
    if i == 6:
        tr.momentum = 0.45      # one step at another momentum, as the momentum correction does
    if i == 7:
        tr.momentum = 0.9


def _same(a, b):
    assert a[3] == b[3]
    for name, x, y in zip(("loss", "weights", "velocity"), a[:3], b[:3]):
        assert torch.equal(x, y), (name, (x.float() - y.float()).abs().max().item())


def test_replays_equal_the_eager_run(cuda, setup):
    state, batches = setup
    eager = _run(cuda, state, batches, None, _hook)
    graph = _run(cuda, state, batches, dict(eager_sightings=2), _hook)
    st = graph[4]
    print(st)
    assert len(st["captured_classes"]) == 1 and st["captures"] == 1 and st["eager_only"] == {}
    assert st["eager_steps"] == 2 and st["replayed_steps"] == STEPS - 2
    assert eager[3] == graph[3] == STEPS
    assert bool(torch.isfinite(eager[0]).all()) and bool(eager[2].any())
    _same(eager, graph)
    # both changes matter: without them the replayed run ends elsewhere (no vacuous pass)
    def lr_only(i, tr):
        if i == 5:
            tr.lr *= 0.1
    plain = _run(cuda, state, batches, dict(eager_sightings=2))
    lr_run = _run(cuda, state, batches, dict(eager_sightings=2), lr_only)
    assert not torch.equal(plain[1], lr_run[1]) and not torch.equal(lr_run[1], graph[1])
