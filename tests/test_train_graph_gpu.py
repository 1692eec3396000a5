"""Training through per-shape-class captured steps (``Trainer.enable_graphs`` / ``train.py --graph``) is BIT-identical
to the eager run: two interleaved shape classes with varying box counts, a learning-rate change after replays have
started (``ReduceLROnPlateau`` sets ``trainer.lr``), weights replaced mid-run (``on_weights_changed``: every graph is
dropped and re-captured) and the cap on captured classes -- through the native RCCL bucket engine (world 1,
``MXR_COMM=native``) with both clip modes -- and the CLI in child processes.  The reference trains at batch 1 per
rank (the reference's train.py:365), where the eager step is bound by the host's kernel issue."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# A: B = 1 at 128 x 192, B: B = 2 at 160 x 128; (class, boxes in gt): the box dimension varies inside one bucket
SEQ = [("A", 3), ("A", 7), ("B", 5), ("A", 4), ("B", 3), ("B", 7), ("A", 5), ("A", 3), ("B", 4), ("A", 7), ("B", 5),
       ("A", 4), ("B", 3), ("A", 5)]
SHAPES = {"A": (1, 128, 192), "B": (2, 160, 128)}


@pytest.fixture(scope="module")
def setup(cuda):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    old = os.environ.get("MXR_COMM")
    os.environ["MXR_COMM"] = "native"
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in models.backbone("resnet18").retinanet(8).state_dict().items()}
    g = torch.Generator().manual_seed(11)
    batches = [{k: v.to(cuda) for k, v in make_batch(*SHAPES[c], num_classes=8, max_boxes=n, generator=g).items()}
               for c, n in SEQ]
    _run(cuda, state, [batches[0], batches[2]], "global", None)      # first sight: the conv tuner races here
    yield state, batches
    if old is None:
        os.environ.pop("MXR_COMM", None)
    else:
        os.environ["MXR_COMM"] = old


def _run(cuda, state, batches, clip_mode, graphs, hook=None):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native
    from batchai_retinanet_horovod_coco_amd.parallel import ops
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    native.set_grad_sinks(None)
    native.set_compute_weights(None)
    model = models.backbone("resnet18").retinanet(8)
    model.load_state_dict(state)
    tr = Trainer(model, lr=1e-4, clipnorm=0.001, compute_dtype=torch.bfloat16, clip_mode=clip_mode, device=cuda,
                 bucket_bytes=4 << 20)
    try:
        assert tr.optimizer.native is not None
        if graphs is not None:
            tr.enable_graphs(**graphs)
        losses = []
        for i, b in enumerate(batches):
            if hook is not None:
                hook(i, tr)
            logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            losses.append(logs["loss"].clone())
        torch.cuda.synchronize()
        stats = tr.step_graphs.stats() if tr.step_graphs is not None else None
        return (torch.stack(losses), tr.flat.data.clone(), tr.base_optimizer.m.clone(), tr.base_optimizer.v.clone(),
                tr.base_optimizer.iterations, stats)
    finally:
        if tr.step_graphs is not None:
            tr.step_graphs.invalidate()
        ops.set_native_comm(None)
        tr.optimizer.native.close()
        native.set_grad_sinks(None)
        native.set_compute_weights(None)


_EAGER = {}


def _eager(cuda, setup, clip_mode, name, n=len(SEQ), hook=None):
    """The all-eager run of a scenario, computed once and shared."""
    key = (clip_mode, name)
    if key not in _EAGER:
        state, batches = setup
        _EAGER[key] = _run(cuda, state, batches[:n], clip_mode, None, hook)
    return _EAGER[key]


def _same(a, b):
    assert a[4] == b[4]
    for name, x, y in zip(("loss", "weights", "adam m", "adam v"), a[:4], b[:4]):
        assert torch.equal(x, y), (name, (x.float() - y.float()).abs().max().item())


CLIP = pytest.mark.parametrize("clip_mode", ["global", "local"])


@CLIP
def test_mixed_shape_classes_are_bit_exact(cuda, setup, clip_mode):
    state, batches = setup
    eager = _eager(cuda, setup, clip_mode, "plain")
    graph = _run(cuda, state, batches, clip_mode, dict(eager_sightings=2))
    st = graph[5]
    print(st)
    assert len(st["captured_classes"]) == 2 and st["replayed_steps"] >= 6 and st["eager_only"] == {}
    assert st["replayed_steps"] + st["eager_steps"] == len(SEQ) == eager[4]
    _same(eager, graph)


@CLIP
def test_learning_rate_change_reaches_the_replays(cuda, setup, clip_mode):
    state, batches = setup

    def drop(i, tr):
        if i == 8:
            tr.lr *= 0.1        # what ReduceLROnPlateau does

    eager = _eager(cuda, setup, clip_mode, "lr", 10, drop)
    graph = _run(cuda, state, batches[:10], clip_mode, dict(eager_sightings=2), drop)
    assert graph[5]["replayed_steps"] >= 4 and len(graph[5]["captured_classes"]) == 2    # steps 8, 9 are replays
    _same(eager, graph)
    unchanged = _run(cuda, state, batches[:10], clip_mode, dict(eager_sightings=2))
    assert not torch.equal(unchanged[1], graph[1])       # the change matters: no vacuous pass


@CLIP
def test_weights_changed_drops_and_recaptures(cuda, setup, clip_mode):
    state, batches = setup

    def halve(i, tr):
        if i == 7:
            tr.flat.data.mul_(0.5)
            tr.on_weights_changed()

    eager = _eager(cuda, setup, clip_mode, "halve", len(SEQ), halve)
    graph = _run(cuda, state, batches, clip_mode, dict(eager_sightings=2), halve)
    st = graph[5]
    print(st)
    assert st["invalidations"] == 1 and st["captures"] >= 3       # 2 before the change, re-captured after it
    _same(eager, graph)


@CLIP
def test_cap_keeps_the_second_class_eager(cuda, setup, clip_mode):
    state, batches = setup
    eager = _eager(cuda, setup, clip_mode, "plain")
    graph = _run(cuda, state, batches, clip_mode, dict(eager_sightings=2, max_shapes=1))
    st = graph[5]
    assert len(st["captured_classes"]) == 1 and len(st["eager_only"]) == 1 and st["replayed_steps"] >= 6
    _same(eager, graph)


# ------------------------------------------------------------------------------------------------ CLI
def _cli(extra, tmp):
    # MXR_CONV_TUNE=0: the first candidate of every key, so two processes run the same kernels (a race's near-ties
    # may differ between processes) and no child spends its time tuning
    env = dict(os.environ, MXR_CONV_TUNE="0", MXR_COMM="native")
    cmd = [sys.executable, "-m", "batchai_retinanet_horovod_coco_amd.bin.train", "--no-weights", "--backbone",
           "resnet18", "--image-min-side", "128", "--image-max-side", "192", "--tensorboard-dir", "", "--seed", "3",
           "--no-evaluation", "--no-snapshots", "--clip-mode", "global"] + extra + \
          ["synthetic", "--num-images", "4", "--height", "128", "--width", "192", "--num-classes", "8",
           "--max-boxes", "4"]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=170)


def test_cli_bench_reports_replays(cuda, tmp_path):
    r = _cli(["--graph", "--bench", "4", "6"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(res["hip_graph"])
    assert res["hip_graph"]["replayed_steps"] >= 6 and res["hip_graph"]["eager_only"] == {}
    assert len(res["hip_graph"]["captured_classes"]) == 1


def test_cli_epoch_losses_match_eager(cuda, tmp_path):
    runs = []
    for name, extra in (("eager", []), ("graph", ["--graph"])):
        path = tmp_path / (name + ".jsonl")
        r = _cli(extra + ["--steps", "6", "--epochs", "2", "--metrics-jsonl", str(path)], tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        recs = [json.loads(l) for l in path.read_text().splitlines()]
        assert len(recs) == 12
        st = [l for l in r.stdout.splitlines() if l.startswith("step graphs: ")]
        assert len(st) == (1 if extra else 0)
        if st:
            assert json.loads(st[0][len("step graphs: "):])["replayed_steps"] >= 6
        runs.append(recs)
    for a, b in zip(*runs):
        assert (a["epoch"], a["step"]) == (b["epoch"], b["step"])
        assert a["loss"] == b["loss"] and a["classification_loss"] == b["classification_loss"], (a, b)
    for ep in (0, 1):
        means = [sum(r["loss"] for r in recs if r["epoch"] == ep) / 6 for recs in runs]
        assert means[0] == means[1]
