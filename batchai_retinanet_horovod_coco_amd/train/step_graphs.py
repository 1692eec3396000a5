"""Per-shape-class HIP-graph replay of the training step (``Trainer.enable_graphs`` / ``train.py --graph``).

The reference job trains at batch 1 per rank (the reference's ``train.py:365``), where the eager step is bound by
the host's kernel issue.  ``Trainer.graph_step`` removes that for ONE batch shape; real batches come in several
padded shape classes and a varying number of ground-truth boxes, the learning rate changes while training
(``ReduceLROnPlateau``), and weights get replaced (broadcast, snapshot restore).  :class:`StepGraphs` keeps one
captured step per shape class and stays bit-identical to the eager run:

* **shape class** = shapes and dtypes of ``images``, ``gt_count``, ``image_hw`` plus gt's box dimension ``G``
  rounded up to a multiple of :data:`G_BUCKET`.  The static gt buffer has the bucket's ``G``; rows past a batch's
  own ``G`` hold -1, and the target kernel reads ``min(gt_count[b], G)`` rows only, so the padding changes nothing.
* **capture policy**: the first ``eager_sightings`` batches of a class are ordinary eager steps (the first one
  tunes, the later ones allocate the lazy state); the next sighting is captured -- which records the step without
  executing it -- and replayed once with that batch.  Every batch is trained on exactly once.  After ``max_shapes``
  captured classes new classes stay eager (no eviction).  Each graph owns its memory pool (replays do not follow
  the capture order).
* **host mirrors**: the capture's Python pass advances ``KerasAdam.iterations`` / ``AdamPlan.host_iter``; they are
  put back after the capture and advanced after every replay.  ``AdamPlan.generation`` only ever grows: one tick
  before a capture (the lazily rebuilt data-gradient weight copies are rebuilt INSIDE the graph), one per replay
  (an eager step after a replay rebuilds them too).
* **learning rate**: written before every replay through ``AdamPlan.set_lr`` (outside the graph), from the same
  expression the eager ``KerasAdam.apply`` uses (``KerasAdam.base_lr``).  ``KerasSGD``'s momentum goes the same way
  (``AdamPlan.set_momentum``).
* **weight EMA** (``ema_decay``): nothing is written before a replay.  The decay cap and ``ema_start`` are by-value
  constants of the captured launch and the decay of each update is derived on the device from the step counter the
  replay advances; a restore that changes them goes through ``on_weights_changed``, which drops every graph.
  ``Trainer.ema_weights()`` exchanges weights and average in place between steps: no pointer moves, no graph goes.
* **lifetime**: the persistent zero-padded gradient rows a captured step writes (``ops.native.ShapeSlots``) are
  pinned while its graph lives; ``Trainer.on_weights_changed`` drops every graph and the classes start over.
* **failure**: a capture that raises, or one in which the conv tuner met a key it still has to race, is thrown
  away: the mirrors are restored, the class is marked eager-only with the reason and the step runs eagerly.
* **multi-rank** (native RCCL bucket engine only, captures only after the first ``TUNER.sync_all``): replayed
  buckets are not registered with the comm watchdog, so before replay n the host waits for replay n-2's done
  event, polling, for at most ``MXR_COMM_TIMEOUT`` seconds, and raises naming the step and the shape class.
"""
from __future__ import annotations

import os
import time
from typing import Dict, Optional, Tuple

import torch

G_BUCKET = 32


def gt_bucket(G: int) -> int:
    """gt's box dimension rounded up to the static buffer's (multiples of :data:`G_BUCKET`, at least one)."""
    return max(1, -(-int(G) // G_BUCKET)) * G_BUCKET


def class_key(images, gt, gt_count, image_hw) -> Tuple:
    return (tuple(images.shape), images.dtype, tuple(gt_count.shape), gt_count.dtype, tuple(image_hw.shape),
            image_hw.dtype, tuple(gt.shape[:1]) + tuple(gt.shape[2:]), gt.dtype, gt_bucket(gt.shape[1]))


class ReplayTimeout(RuntimeError):
    pass


class HipGraphBackend:
    """The device side of :class:`StepGraphs`: static input buffers, capture / replay, done events, the tuner."""

    def __init__(self, device):
        self.device = device

    def ready(self) -> Optional[str]:
        """None when a capture may happen now, else why not yet (the class keeps running eagerly, unmarked)."""
        from ..parallel import runtime
        if runtime.is_initialized() and runtime.distributed():
            from ..ops.conv_tuner import TUNER
            if TUNER.syncs == 0:
                return "waiting for the first conv-table merge across ranks"
        return None

    def bounded(self) -> bool:
        from ..parallel import runtime
        return runtime.is_initialized() and runtime.distributed()

    def tuner_misses(self) -> int:
        from ..ops.conv_tuner import TUNER
        return len(TUNER.capture_misses)

    def last_miss(self) -> str:
        from ..ops.conv_tuner import TUNER
        return TUNER.capture_misses[-1] if TUNER.capture_misses else ""

    def static_inputs(self, images, gt, gt_count, image_hw, G: int) -> Dict[str, torch.Tensor]:
        dev = self.device
        sgt = torch.full((gt.shape[0], G) + tuple(gt.shape[2:]), -1.0, dtype=gt.dtype, device=dev)
        return {"images": torch.empty(images.shape, dtype=images.dtype, device=dev), "gt": sgt,
                "gt_count": torch.empty(gt_count.shape, dtype=gt_count.dtype, device=dev),
                "image_hw": torch.empty(image_hw.shape, dtype=image_hw.dtype, device=dev)}

    def load(self, static, images, gt, gt_count, image_hw) -> None:
        static["images"].copy_(images, non_blocking=True)
        sgt = static["gt"]
        if gt.shape[1] != sgt.shape[1]:
            sgt.fill_(-1.0)
            sgt = sgt[:, :gt.shape[1]]
        sgt.copy_(gt, non_blocking=True)
        static["gt_count"].copy_(gt_count, non_blocking=True)
        static["image_hw"].copy_(image_hw, non_blocking=True)

    def capture(self, step, static):
        """Record ``step(**static)`` (not executed).  Returns (graph, logs): ``logs`` are the step's loss scalars
        stacked in one static tensor."""
        graph = torch.cuda.CUDAGraph()
        # thread-local capture: the comm engine's watchdog thread may still poll an earlier step's events;
        # no shared pool: every graph allocates from a private one, since replays do not follow the capture order
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            logs = step(**static)
            names = tuple(logs)
            out = torch.stack([logs[k].reshape(()).float() for k in names])
        return graph, (names, out)

    def replay(self, graph, logs) -> Dict[str, torch.Tensor]:
        graph.replay()
        names, out = logs
        return dict(zip(names, out.clone().unbind(0)))     # a replay overwrites the static scalars: hand out copies

    def event(self):
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def release(self, graph) -> None:
        torch.cuda.current_stream(self.device).synchronize()     # no replay of it in flight when its pool goes


class _Class:
    __slots__ = ("key", "sightings", "graph", "logs", "static", "eager_reason", "replays", "captures")

    def __init__(self, key):
        self.key = key
        self.sightings = 0
        self.graph = self.logs = self.static = None
        self.eager_reason: Optional[str] = None
        self.replays = 0
        self.captures = 0

    def name(self) -> str:
        k = self.key
        return "images{}/G{}".format("x".join(str(v) for v in k[0]), k[-1])


class StepGraphs:
    def __init__(self, trainer, max_shapes: int = 8, eager_sightings: int = 2, backend=None,
                 timeout_s: Optional[float] = None, clock=time.monotonic, sleep=time.sleep):
        self.trainer = trainer
        self.max_shapes = int(max_shapes)
        self.eager_sightings = int(eager_sightings)
        self.backend = backend if backend is not None else HipGraphBackend(trainer.device)
        self.timeout_s = float(os.environ.get("MXR_COMM_TIMEOUT", "600")) if timeout_s is None else float(timeout_s)
        self.clock, self.sleep = clock, sleep
        self.classes: Dict[Tuple, _Class] = {}
        self.replayed = self.eager = self.captured_total = self.invalidations = 0
        self._done = []         # (step number, class name, done event) of the last two replays
        self._step = 0

    # ------------------------------------------------------------------ public
    def captured(self) -> int:
        return sum(1 for e in self.classes.values() if e.graph is not None)

    def stats(self) -> dict:
        return {"captured_classes": [e.name() for e in self.classes.values() if e.graph is not None],
                "captures": self.captured_total, "replayed_steps": self.replayed, "eager_steps": self.eager,
                "eager_only": {e.name(): e.eager_reason for e in self.classes.values() if e.eager_reason},
                "invalidations": self.invalidations, "max_shapes": self.max_shapes,
                "eager_sightings": self.eager_sightings}

    def invalidate(self) -> None:
        """Drop every graph (weights / optimizer state were replaced under them); the classes start over."""
        had = [e for e in self.classes.values() if e.graph is not None]
        for e in had:
            self.backend.release(e.graph)
        if had or self.classes:
            self.invalidations += 1
        self.classes = {}
        self._done = []
        for s in self.trainer.persistent_slots():
            s.unpin_all()

    def step(self, images, gt, gt_count, image_hw):
        key = class_key(images, gt, gt_count, image_hw)
        e = self.classes.get(key)
        if e is None:
            e = self.classes[key] = _Class(key)
        self._step += 1
        if e.graph is None and e.eager_reason is None and e.sightings >= self.eager_sightings:
            if self.captured() >= self.max_shapes:
                e.eager_reason = "max_shapes ({}) classes already captured".format(self.max_shapes)
            elif self.backend.ready() is None:
                self._capture(e, images, gt, gt_count, image_hw)
        if e.graph is not None:
            return self._replay(e, images, gt, gt_count, image_hw)
        e.sightings += 1
        self.eager += 1
        return self.trainer._train_on_batch(images, gt, gt_count, image_hw)

    # ------------------------------------------------------------------ capture / replay
    def _capture(self, e: _Class, images, gt, gt_count, image_hw) -> bool:
        tr, be = self.trainer, self.backend
        opt, plan = tr.base_optimizer, tr.adam_plan()
        it0 = opt.iterations
        if plan is not None:
            # nothing of the host-side Adam bookkeeping may turn into a graph node: the device step counter and
            # the lr are brought up to date eagerly, so the captured pass finds them current
            plan.sync_iter(it0)
            plan.set_lr(opt.base_lr(it0 + 1))
            if hasattr(opt, "momentum"):
                plan.set_momentum(opt.momentum)
            plan.generation += 1        # the lazily rebuilt weight copies are rebuilt inside the graph
        misses0 = be.tuner_misses()
        reason = None
        graph = logs = static = None
        try:
            static = be.static_inputs(images, gt, gt_count, image_hw, key_G(e.key))
            graph, logs = be.capture(tr._train_on_batch, static)
            if be.tuner_misses() != misses0:
                reason = "the conv tuner still has to race a key of this class ({})".format(be.last_miss())
        except RuntimeError as exc:
            reason = "capture failed: {}".format(str(exc).splitlines()[0][:160] if str(exc) else type(exc).__name__)
        # capturing records the step without executing it, but the host counters advanced while the Python ran
        opt.iterations = it0
        if plan is not None:
            plan.host_iter = it0
            if reason is not None:
                plan.generation += 1    # whatever the abandoned pass marked as rebuilt was not
        if reason is not None:
            if graph is not None:
                be.release(graph)
            e.eager_reason = reason
            return False
        for s in tr.persistent_slots():
            s.pin_current()
        e.graph, e.logs, e.static = graph, logs, static
        e.captures += 1
        self.captured_total += 1
        return True

    def _replay(self, e: _Class, images, gt, gt_count, image_hw):
        tr, be = self.trainer, self.backend
        opt, plan = tr.base_optimizer, tr.adam_plan()
        if be.bounded():
            self._bound_run_ahead()
        be.load(e.static, images, gt, gt_count, image_hw)
        if plan is not None:
            plan.sync_iter(opt.iterations)
            plan.set_lr(opt.base_lr(opt.iterations + 1))
            if hasattr(opt, "momentum"):
                plan.set_momentum(opt.momentum)     # SGD: hyper[2], read by the replayed kernel
        logs = be.replay(e.graph, e.logs)
        # the captured Adam advanced the device step counter and rewrote the compute weights
        opt.iterations += 1
        if plan is not None:
            plan.host_iter += 1
            plan.generation += 1
        if be.bounded():
            self._done.append((self._step, e.name(), be.event()))
        e.replays += 1
        self.replayed += 1
        tr.last_logs = logs
        return logs

    def _bound_run_ahead(self) -> None:
        """Before launching a replay, replay n-2 must be done: a bounded, polling wait (a replayed all-reduce that
        never completes is seen here, not by the comm watchdog), which also caps the host's run-ahead at two."""
        while len(self._done) >= 2:
            step, name, ev = self._done[0]
            deadline = self.clock() + self.timeout_s
            while not ev.query():
                if self.clock() > deadline:
                    raise ReplayTimeout("graph replay of step {} (shape class {}) did not complete within {:g} s "
                                        "(MXR_COMM_TIMEOUT): a collective inside the replay is stuck"
                                        .format(step, name, self.timeout_s))
                self.sleep(0.0002)
            self._done.pop(0)


def key_G(key) -> int:
    return key[-1]
