"""``Trainer(regression_loss="giou")`` through captured steps (``Trainer.enable_graphs``) is BIT-identical to the eager
run (the IoU kernel reads the anchor cache's persistent tensor, so a replay holds a valid pointer); naming
``regression_loss="smooth_l1"`` is bit-identical to not passing the argument; and the regression loss a step logs
(the HIP kernel) agrees with ``forward_losses`` (the torch expression) on the same weights and batch.  Setup as in
test_sgd_graph_gpu.py: resnet18, 8 classes, one 128 x 192 image per batch, bf16, a first eager sight that tunes."""
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
    _run(cuda, state, batches[:1], None, regression_loss="giou")      # first sight: the conv tuner races here
    return state, batches


def _trainer(cuda, state, **kw):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    native.set_grad_sinks(None)
    native.set_compute_weights(None)
    model = models.backbone("resnet18").retinanet(8)
    model.load_state_dict(state)
    return Trainer(model, lr=1e-3, clipnorm=10.0, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda, **kw)


def _release(tr):
    from batchai_retinanet_horovod_coco_amd.ops import native
    if tr.step_graphs is not None:
        tr.step_graphs.invalidate()
    native.set_grad_sinks(None)
    native.set_compute_weights(None)


def _run(cuda, state, batches, graphs, **kw):
    tr = _trainer(cuda, state, **kw)
    try:
        assert tr.adam_plan() is not None
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


def test_giou_replays_equal_the_eager_run(cuda, setup):
    state, batches = setup
    eager = _run(cuda, state, batches, None, regression_loss="giou")
    graph = _run(cuda, state, batches, dict(eager_sightings=2), regression_loss="giou")
    st = graph[5]
    print(st)
    assert len(st["captured_classes"]) == 1 and st["captures"] == 1 and st["eager_only"] == {}
    assert st["eager_steps"] == 2 and st["replayed_steps"] == STEPS - 2
    assert eager[4] == graph[4] == STEPS
    assert bool(torch.isfinite(eager[0]).all()) and bool((eager[0][:, 1] > 0).all()) and bool(eager[2].any())
    _same(eager, graph)
    # the loss matters: the smooth-L1 run ends elsewhere (no vacuous pass)
    plain = _run(cuda, state, batches, dict(eager_sightings=2))
    assert not torch.equal(plain[1], graph[1]) and not torch.equal(plain[0][:, 1], graph[0][:, 1])


def test_naming_smooth_l1_changes_nothing(cuda, setup):
    state, batches = setup
    _same(_run(cuda, state, batches[:4], None), _run(cuda, state, batches[:4], None, regression_loss="smooth_l1"))


def _logged_against_torch(cuda, state, b, **kw):
    """|logged - torch| / torch of one step's regression loss: the HIP kernel inside train_on_batch against
    forward_losses (the torch expression) on the weights the step started from."""
    tr = _trainer(cuda, state, **kw)
    try:
        want = tr.forward_losses(b["images"], b["gt"], b["gt_count"], b["image_hw"])[0].double().item()
        got = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])["regression_loss"].double().item()
        torch.cuda.synchronize()
    finally:
        _release(tr)
    assert want > 0 and got > 0
    return abs(got - want) / want, got, want


def test_logged_loss_agrees_with_the_torch_expression(cuda, setup):
    """Both paths share the bf16 forward, so they differ by the loss arithmetic alone (fp32, another order of
    summation).  The yardstick is measured here: the same comparison for smooth-L1; the GIoU arm may differ by at
    most twice that.  On an MI355X both arms agree bit for bit on this batch (smooth-L1 68.07616424560547, GIoU
    1.2735081911087036 from either path)."""
    state, batches = setup
    b = batches[1]          # 7 boxes
    sl1 = _logged_against_torch(cuda, state, b)
    giou = _logged_against_torch(cuda, state, b, regression_loss="giou")
    print("smooth_l1: logged {!r} torch {!r} rel {:.3e}".format(sl1[1], sl1[2], sl1[0]))
    print("giou:      logged {!r} torch {!r} rel {:.3e}".format(giou[1], giou[2], giou[0]))
    assert giou[0] <= 2 * sl1[0], (giou, sl1)
