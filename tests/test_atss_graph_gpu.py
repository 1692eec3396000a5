"""``Trainer(assigner="atss")`` through captured steps (``Trainer.enable_graphs``) is BIT-identical to the eager run over
batches whose box counts differ within one G bucket (the ATSS kernels read ``gt_count`` on the device and never a row
at or beyond it, and their grids depend on B, G and A alone, so a replay with other boxes is the eager step); naming
``assigner="iou"`` is bit-identical to not passing the argument; and the HIP and torch target backends give the same
state on integer-corner boxes.  Setup as in test_iou_loss_graph_gpu.py: resnet18, 8 classes, one 128 x 192 image per
batch, bf16, a first eager sight that tunes."""
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
    # one G bucket (train.step_graphs.G_BUCKET = 32): the eager steps see G = 3..7 rows, the replays the static
    # buffer's 32, padded with -1 rows that must not be read, under box counts that change from batch to batch
    assert len({int(b["gt_count"][0]) for b in batches}) > 1 and len({b["gt"].shape[1] for b in batches}) > 1
    _run(cuda, state, batches[:1], None, assigner="atss")      # first sight: the conv tuner races here
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


def test_atss_replays_equal_the_eager_run(cuda, setup):
    state, batches = setup
    eager = _run(cuda, state, batches, None, assigner="atss")
    graph = _run(cuda, state, batches, dict(eager_sightings=2), assigner="atss")
    st = graph[5]
    print(st)
    assert len(st["captured_classes"]) == 1 and st["captures"] == 1 and st["eager_only"] == {}
    assert st["eager_steps"] == 2 and st["replayed_steps"] == STEPS - 2
    assert eager[4] == graph[4] == STEPS
    assert bool(torch.isfinite(eager[0]).all()) and bool((eager[0][:, 1] > 0).all()) and bool(eager[2].any())
    _same(eager, graph)
    # the assigner matters: the fixed-threshold run ends elsewhere (no vacuous pass)
    plain = _run(cuda, state, batches, dict(eager_sightings=2))
    assert not torch.equal(plain[1], graph[1]) and not torch.equal(plain[0][:, 1], graph[0][:, 1])


def test_naming_iou_changes_nothing(cuda, setup):
    state, batches = setup
    _same(_run(cuda, state, batches[:4], None), _run(cuda, state, batches[:4], None, assigner="iou"))


def test_hip_and_torch_backends_give_the_same_state(cuda, setup):
    """Boxes rounded to integer corners: every distance is exact in fp32, so both backends select the same
    candidates and compute the same IoUs from the same fp32 expression; only the order of summation in a threshold
    differs (1e-7); the float64 oracle's IoUs of these six boxes stay 1.0e-4 away from their thresholds."""
    state, batches = setup
    b = batches[1]                          # 6 boxes in 7 rows
    gt = b["gt"].clone()
    n = int(b["gt_count"][0])
    gt[:, :n, :4] = gt[:, :n, :4].round()
    assert bool((gt[0, :n, 2] > gt[0, :n, 0]).all()) and bool((gt[0, :n, 3] > gt[0, :n, 1]).all())
    out = {}
    for backend in ("hip", "torch"):
        tr = _trainer(cuda, state, assigner="atss", target_backend=backend)
        try:
            out[backend] = tr.compute_targets(b["images"], gt, b["gt_count"], b["image_hw"])
            torch.cuda.synchronize()
        finally:
            _release(tr)
    hip, ref = out["hip"], out["torch"]
    assert torch.equal(hip[0], ref[0]) and torch.equal(hip[1], ref[1]) and torch.equal(hip[3], ref[3])
    pos = hip[0] == 1
    assert hip[3].item() == int(pos.sum()) > 0
    assert torch.allclose(hip[2][pos], ref[2][pos], rtol=1e-5, atol=1e-6)
    assert not bool(hip[2][~pos].any()) and not bool(ref[2][~pos].any())
