"""``RetinaNet(regression_bins=17)`` with ``giou`` and ``qfl`` through captured steps (``Trainer.enable_graphs``) is
BIT-identical to the eager run over two batch shapes (the grids of box_dist.hip depend on the row count and the bin
count alone, and the kernels use no atomics, so a replay computes what the eager step computes);
``regression_bins=0`` -- what ``--regression-bins 0`` resolves to -- is bit-identical to not naming it, with the same
parameter count; and the losses a step logs agree with ``forward_losses`` on the same weights and batch.  Setup as in
test_group_norm_graph_gpu.py: resnet18, 8 classes, one image per batch, bf16, a first eager sight that tunes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(128, 192), (160, 160)]
BOXES = [3, 7, 5, 4, 3, 7, 5, 4]
STEPS = len(BOXES)
# both paths share the bf16 forward, so the logged losses (the fused kernels) and forward_losses (the torch
# expressions) differ by the loss arithmetic alone: the bound test_group_norm_graph_gpu.py holds two fp32 sums to
TWO_LOSS_RTOL = 2e-5
DIST = dict(regression_bins=17)
LOSSES = dict(regression_loss="giou", classification_loss="qfl")


@pytest.fixture(scope="module")
def setup(cuda):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.bin import train as T
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    torch.manual_seed(0)
    plain = {k: v.clone() for k, v in models.backbone("resnet18").retinanet(8).state_dict().items()}
    torch.manual_seed(0)
    dist = {k: v.clone() for k, v in models.backbone("resnet18").retinanet(8, **DIST).state_dict().items()}
    g = torch.Generator().manual_seed(12)
    batches = []
    for i, n in enumerate(BOXES):
        h, w = SHAPES[i % 2]
        batches.append({k: v.to(cuda) for k, v in make_batch(1, h, w, num_classes=8, max_boxes=n, generator=g).items()})
    _run(cuda, dist, batches[:2], None, DIST)       # first sight of both shapes: the conv tuner races here
    return plain, dist, batches, T


def _trainer(cuda, state, model_kw, **kw):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    native.set_grad_sinks(None)
    native.set_compute_weights(None)
    model = models.backbone("resnet18").retinanet(8, **(model_kw or {}))
    model.load_state_dict(state)
    return Trainer(model, lr=1e-3, clipnorm=10.0, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda,
                   **dict(LOSSES, **kw))


def _release(tr):
    from batchai_retinanet_horovod_coco_amd.ops import native
    if tr.step_graphs is not None:
        tr.step_graphs.invalidate()
    native.set_grad_sinks(None)
    native.set_compute_weights(None)


def _run(cuda, state, batches, graphs, model_kw):
    tr = _trainer(cuda, state, model_kw)
    try:
        if graphs is not None:
            tr.enable_graphs(**graphs)
        losses = []
        for b in batches:
            logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            losses.append(torch.stack([logs["loss"], logs["regression_loss"], logs["classification_loss"]]).clone())
        torch.cuda.synchronize()
        opt = tr.base_optimizer
        stats = tr.step_graphs.stats() if tr.step_graphs is not None else None
        return torch.stack(losses), tr.flat.data.clone(), opt.m.clone(), opt.v.clone(), opt.iterations, stats
    finally:
        _release(tr)


def _same(a, b):
    assert a[4] == b[4]
    for name, x, y in zip(("losses", "weights", "m", "v"), a[:4], b[:4]):
        assert torch.equal(x, y), (name, (x.float() - y.float()).abs().max().item())


def test_replays_equal_the_eager_run(cuda, setup):
    plain_state, state, batches, _ = setup
    eager = _run(cuda, state, batches, None, DIST)
    graph = _run(cuda, state, batches, dict(eager_sightings=2), DIST)
    st = graph[5]
    print(st)
    assert len(st["captured_classes"]) == 2 and st["captures"] == 2 and st["eager_only"] == {}
    assert st["eager_steps"] == 4 and st["replayed_steps"] == STEPS - 4
    assert eager[4] == graph[4] == STEPS
    assert bool(torch.isfinite(eager[0]).all()) and bool(eager[2].any())
    _same(eager, graph)
    # the head matters: the 4-number head under the same losses ends elsewhere (no vacuous pass)
    plain = _run(cuda, plain_state, batches, dict(eager_sightings=2), None)
    assert plain[1].numel() < graph[1].numel()
    assert not torch.equal(plain[0], graph[0])


def test_naming_zero_bins_changes_nothing(cuda, setup):
    plain_state, _, batches, T = setup
    a = T.parse_args(["--regression-bins", "0", "coco", "/x"])
    assert T.regression_bins_kwargs(a) == T.regression_bins_kwargs(T.parse_args(["coco", "/x"])) == {}
    default = _run(cuda, plain_state, batches[:4], None, None)
    named = _run(cuda, plain_state, batches[:4], None, dict(regression_bins=0))
    assert default[1].numel() == named[1].numel()       # no new parameter
    _same(default, named)


def test_logged_losses_agree_with_forward_losses(cuda, setup):
    _, state, batches, _ = setup
    b = batches[1]          # 7 boxes
    tr = _trainer(cuda, state, DIST)
    try:
        want = [v.double().item() for v in tr.forward_losses(b["images"], b["gt"], b["gt_count"], b["image_hw"])]
        logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
        got = [logs["regression_loss"].double().item(), logs["classification_loss"].double().item()]
        torch.cuda.synchronize()
    finally:
        _release(tr)
    for name, g, w in zip(("regression", "classification"), got, want):
        print("{}: logged {!r} forward_losses {!r} rel {:.3e}".format(name, g, w, abs(g - w) / w))
        assert w > 0 and abs(g - w) <= TWO_LOSS_RTOL * w
