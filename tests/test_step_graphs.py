"""The per-shape-class step-graph cache (train/step_graphs.py) against a fake trainer and capture backend: the
policy -- eager sightings, capture on the next one, gt bucketing, the cap, invalidation, failure handling, the
bounded replay wait -- needs no GPU.  Plus the CLI surface of ``--graph``."""
import json

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.train.step_graphs import ReplayTimeout, StepGraphs, class_key, gt_bucket


class FakePlan:
    def __init__(self):
        self.host_iter = 0
        self.generation = 0
        self.lrs = []

    def set_lr(self, lr):
        self.lrs.append(lr)

    def sync_iter(self, it):
        self.host_iter = it


class FakeOpt:
    def __init__(self):
        self.iterations = 0
        self.lr = 1e-3
        self.decay = 0.5

    def base_lr(self, t):
        return self.lr / (1.0 + self.decay * (t - 1))


class FakeSlots:
    def __init__(self):
        self.pins = self.unpins = 0

    def pin_current(self):
        self.pins += 1

    def unpin_all(self):
        self.unpins += 1


class FakeTrainer:
    device = torch.device("cpu")

    def __init__(self):
        self.base_optimizer = FakeOpt()
        self.plan = FakePlan()
        self.slots = FakeSlots()
        self.trained = []           # (path, sum of the images) per executed step
        self.recording = False
        self.last_logs = None

    def adam_plan(self):
        return self.plan

    def persistent_slots(self):
        return [self.slots]

    def _train_on_batch(self, images, gt, gt_count, image_hw):
        # the host side of a step: the mirrors advance whether the step executes or is only recorded
        self.base_optimizer.iterations += 1
        self.plan.host_iter += 1
        self.plan.generation += 1
        if not self.recording:
            self.trained.append(("eager", float(images.sum()), int(gt.shape[1])))
        return {"loss": images.sum() * 0 + self.base_optimizer.iterations}


class FakeEvent:
    def __init__(self, done):
        self.done = done

    def query(self):
        return self.done


class FakeBackend:
    def __init__(self, trainer, fail=None, miss=False, bounded=False, events_done=True, ready=None):
        self.tr, self.fail, self.miss, self._bounded, self.events_done = trainer, fail, miss, bounded, events_done
        self._ready = ready
        self.misses = 0
        self.released = 0

    def ready(self):
        return self._ready

    def bounded(self):
        return self._bounded

    def tuner_misses(self):
        return self.misses

    def last_miss(self):
        return "wgrad|fake"

    def static_inputs(self, images, gt, gt_count, image_hw, G):
        return {"images": torch.empty_like(images), "gt": torch.full((gt.shape[0], G, 5), -1.0),
                "gt_count": torch.empty_like(gt_count), "image_hw": torch.empty_like(image_hw)}

    def load(self, static, images, gt, gt_count, image_hw):
        static["images"].copy_(images)
        static["gt"].fill_(-1.0)
        static["gt"][:, :gt.shape[1]].copy_(gt)

    def capture(self, step, static):
        self.tr.recording = True
        try:
            step(**static)
            if self.fail:
                raise RuntimeError(self.fail)
            if self.miss:
                self.misses += 1
        finally:
            self.tr.recording = False
        return object(), static

    def replay(self, graph, static):
        self.tr.trained.append(("replay", float(static["images"].sum()), int(static["gt"].shape[1])))
        return {"loss": torch.tensor(float(self.tr.base_optimizer.iterations + 1))}

    def event(self):
        return FakeEvent(self.events_done)

    def release(self, graph):
        self.released += 1


def batch(i, B=1, H=8, W=8, G=3):
    return (torch.full((B, H, W, 3), float(i)), torch.zeros((B, G, 5)), torch.ones((B,), dtype=torch.int32),
            torch.tensor([[H, W]] * B, dtype=torch.int32))


def make(**kw):
    tr = FakeTrainer()
    be_kw = {k: kw.pop(k) for k in list(kw) if k in ("fail", "miss", "bounded", "events_done", "ready")}
    sg = StepGraphs(tr, backend=FakeBackend(tr, **be_kw), **kw)
    return tr, sg


def test_gt_bucketing():
    assert [gt_bucket(g) for g in (0, 1, 3, 7, 32, 33, 40, 64, 65)] == [32, 32, 32, 32, 32, 64, 64, 64, 96]
    k3, k7, k40 = (class_key(*batch(0, G=g)) for g in (3, 7, 40))
    assert k3 == k7 and k3 != k40
    assert class_key(*batch(0, B=2)) != k3 and class_key(*batch(0, H=16)) != k3


def test_sightings_then_capture_and_every_batch_trained_once():
    tr, sg = make(eager_sightings=2)
    for i in range(1, 7):
        logs = sg.step(*batch(i, G=3 if i % 2 else 7))
        assert float(logs["loss"]) == i                  # the step number the eager run would report
        assert tr.base_optimizer.iterations == tr.plan.host_iter == i
    # two eager sightings, capture + first replay on the third, and each batch trained on exactly once, in order
    assert [p for p, _, _ in tr.trained] == ["eager", "eager", "replay", "replay", "replay", "replay"]
    assert [v for _, v, _ in tr.trained] == [float(i) * 8 * 8 * 3 for i in range(1, 7)]
    assert all(g == 32 for p, _, g in tr.trained if p == "replay")       # the bucket's static gt
    st = sg.stats()
    assert st["replayed_steps"] == 4 and st["eager_steps"] == 2 and len(st["captured_classes"]) == 1
    assert st["captures"] == 1 and st["eager_only"] == {} and tr.slots.pins == 1


def test_lr_written_before_every_replay_with_decay():
    tr, sg = make(eager_sightings=1)
    sg.step(*batch(1))
    sg.step(*batch(2))            # capture (lr of iteration 2 made current) + replay
    tr.base_optimizer.lr = 1e-4   # ReduceLROnPlateau
    sg.step(*batch(3))
    opt = tr.base_optimizer
    assert tr.plan.lrs[-1] == pytest.approx(1e-4 / (1.0 + 0.5 * 2))
    assert tr.plan.lrs[-2] == pytest.approx(1e-3 / (1.0 + 0.5 * 1))
    assert opt.iterations == 3


def test_generation_only_grows_and_ticks_per_replay():
    tr, sg = make(eager_sightings=1)
    gens = []
    for i in range(1, 5):
        sg.step(*batch(i))
        gens.append(tr.plan.generation)
    assert all(b > a for a, b in zip(gens, gens[1:])), gens


def test_more_boxes_than_the_bucket_is_a_new_class():
    tr, sg = make(eager_sightings=1)
    for i, g in enumerate((3, 7, 5, 40, 33, 64), 1):
        sg.step(*batch(i, G=g))
    assert len(sg.stats()["captured_classes"]) == 2
    assert [p for p, _, _ in tr.trained] == ["eager", "replay", "replay", "eager", "replay", "replay"]


def test_cap_keeps_new_classes_eager():
    tr, sg = make(eager_sightings=1, max_shapes=1)
    for i in range(1, 4):
        sg.step(*batch(i))
    for i in range(4, 8):
        sg.step(*batch(i, H=16))
    st = sg.stats()
    assert len(st["captured_classes"]) == 1 and st["replayed_steps"] == 2 and st["eager_steps"] == 5
    assert list(st["eager_only"].values()) == ["max_shapes (1) classes already captured"]
    assert tr.base_optimizer.iterations == 7


def test_on_weights_changed_drops_graphs_and_sightings_restart():
    tr, sg = make(eager_sightings=2)
    for i in range(1, 5):
        sg.step(*batch(i))
    assert sg.captured() == 1
    sg.invalidate()
    assert sg.captured() == 0 and sg.backend.released == 1 and tr.slots.unpins == 1
    for i in range(5, 9):
        sg.step(*batch(i))
    assert [p for p, _, _ in tr.trained] == ["eager", "eager", "replay", "replay"] * 2
    st = sg.stats()
    assert st["captures"] == 2 and st["invalidations"] == 1 and len(st["captured_classes"]) == 1


def test_trainer_on_weights_changed_invalidates():
    """The real Trainer routes train_on_batch through the cache and drops it in on_weights_changed."""
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    tr = Trainer(models.backbone("resnet18").retinanet(2), device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="GPU"):
        tr.enable_graphs()
    calls = []

    class Spy:
        def step(self, *a):
            calls.append("step")
            return {}

        def invalidate(self):
            calls.append("invalidate")
    tr.step_graphs = Spy()
    tr.train_on_batch(*batch(1))
    tr.on_weights_changed()
    assert calls == ["step", "invalidate"]


@pytest.mark.parametrize("kw, why", [({"fail": "hipErrorStreamCaptureUnsupported: library kernel"}, "capture failed"),
                                     ({"miss": True}, "still has to race")])
def test_failed_capture_restores_mirrors_and_marks_eager_only(kw, why):
    tr, sg = make(eager_sightings=1, **kw)
    for i in range(1, 5):
        logs = sg.step(*batch(i))
        assert float(logs["loss"]) == i
        assert tr.base_optimizer.iterations == tr.plan.host_iter == i
    assert [p for p, _, _ in tr.trained] == ["eager"] * 4        # the trainer stays usable, every batch trained once
    st = sg.stats()
    assert st["captured_classes"] == [] and st["eager_steps"] == 4 and st["replayed_steps"] == 0
    (reason,) = st["eager_only"].values()
    assert why in reason
    assert tr.slots.pins == 0 and sg.backend.released == (1 if "miss" in kw else 0)


def test_not_ready_stays_eager_without_a_mark():
    tr, sg = make(eager_sightings=1, ready="waiting for the first conv-table merge across ranks")
    for i in range(1, 4):
        sg.step(*batch(i))
    assert sg.stats()["eager_only"] == {} and sg.stats()["eager_steps"] == 3
    sg.backend._ready = None
    sg.step(*batch(4))
    assert sg.stats()["replayed_steps"] == 1


def test_bounded_wait_raises_naming_step_and_class():
    now = [0.0]

    def sleep(dt):
        now[0] += 1.0           # a fake clock: no test time passes

    tr, sg = make(eager_sightings=0, bounded=True, events_done=False, timeout_s=5.0, clock=lambda: now[0], sleep=sleep)
    sg.step(*batch(1))
    sg.step(*batch(2))          # two replays in flight are allowed
    with pytest.raises(ReplayTimeout, match=r"step 1 \(shape class images1x8x8x3/G32\).*5 s"):
        sg.step(*batch(3))
    assert now[0] <= 7.0


def test_bounded_wait_passes_completed_replays():
    tr, sg = make(eager_sightings=0, bounded=True, events_done=True, timeout_s=5.0)
    for i in range(1, 6):
        sg.step(*batch(i))
    assert sg.stats()["replayed_steps"] == 5 and len(sg._done) == 2


# ------------------------------------------------------------------------------------------------ CLI
def test_parse_args_graph_flags():
    a = T.parse_args(["synthetic"])
    assert a.graph is False and a.graph_shapes == 8
    a = T.parse_args(["--graph", "--graph-shapes", "3", "synthetic"])
    assert a.graph is True and a.graph_shapes == 3


def test_graph_with_fp8_is_refused():
    with pytest.raises(SystemExit, match="fp8"):
        T.parse_args(["--graph", "--dtype", "fp8", "synthetic"])
    T.parse_args(["--dtype", "fp8", "synthetic"])        # fp8 alone is still accepted


def test_graph_on_cpu_runs_eagerly(tmp_path, capsys):
    rc = T.main(["--no-weights", "--backbone", "resnet18", "--image-min-side", "64", "--image-max-side", "64",
                 "--device", "cpu", "--graph", "--bench", "1", "2", "--no-evaluation", "--seed", "1",
                 "synthetic", "--num-images", "2", "--height", "64", "--width", "64", "--num-classes", "4",
                 "--max-boxes", "3"])
    assert rc == 0
    out = capsys.readouterr().out.splitlines()
    assert sum("--graph" in l and "eagerly" in l for l in out) == 1
    res = json.loads([l for l in out if l.startswith("{")][-1])
    assert res["hip_graph"] is False and res["steps"] == 2
