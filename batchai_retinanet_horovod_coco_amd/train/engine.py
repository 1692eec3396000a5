"""One training step: targets -> forward -> focal + smooth-L1 -> backward -> reduce/clip/Adam.

This is CS3 of the survey (the hot loop of ``fit_generator`` driven from
``/root/reference/train.py:444-450``), re-planned for one MI355X per process:

* batches arrive as device tensors: images (B, H, W, 3) and padded gt boxes (B, G, 5);
  anchor targets are computed ON the device (fused HIP kernel), so only kilobytes of boxes
  cross PCIe instead of the reference's 65 MB/image one-hot labels;
* the forward runs NHWC in the compute dtype (bf16 on MI355X) against fp32 master weights;
* losses are fused sigmoid-focal / smooth-L1 kernels that also emit the logit gradients;
* gradients land in the flat fp32 buffer, get all-reduced in buckets (overlapped with the
  backward when ``clip_mode='global'``), and one fused kernel does clip + Adam.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional

import torch

from ..ops import anchors as anchor_ops
from ..ops import losses
from ..parallel import runtime
from ..parallel.distributed_optimizer import DistributedOptimizer
from .flat import FlatParams, backward_order
from .optimizer import KerasAdam, KerasSGD


_ROCTX = os.environ.get("MXR_ROCTX", "0") == "1"


class _range:
    """roctx range (``MXR_ROCTX=1``; visible in rocprofv3 --marker-trace / sys-trace)."""

    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        if _ROCTX and torch.cuda.is_available():
            torch.cuda.nvtx.range_push(self.name)
        return self

    def __exit__(self, *a):
        if _ROCTX and torch.cuda.is_available():
            torch.cuda.nvtx.range_pop()


# MXR_PAD_FOCAL=0: hand autograd plain (B, A, C) classification / regression gradients (the final layers pad them)
_PAD_FOCAL = os.environ.get("MXR_PAD_FOCAL", "1") == "1"

class Trainer:
    def __init__(self, model, lr: float = 1e-5, clipnorm: float = 0.001, compute_dtype: torch.dtype = torch.float32,
                 clip_mode: str = "local", compression=None, bucket_bytes: Optional[int] = None,
                 device: Optional[torch.device] = None, overlap: bool = True, target_backend: str = "auto",
                 optimizer: str = "adam", momentum: float = 0.0, nesterov: bool = False, weight_decay: float = 0.0,
                 ema_decay: float = 0.0, regression_loss: str = "smooth_l1", regression_weight: float = 1.0,
                 assigner: str = "iou", atss_topk: int = anchor_ops.ATSS_TOPK, classification_loss: str = "focal",
                 dfl_weight: float = losses.DFL_WEIGHT):
        from ..parallel.collectives import Compression
        # a distribution box head (RetinaNet(regression_bins=K)): the box loss on its integral deltas plus DFL
        self.regression_bins = int(getattr(model, "regression_bins", 0) or 0)
        self.regression_range = float(getattr(model, "regression_range", 8.0))
        if not self.regression_bins and dfl_weight != losses.DFL_WEIGHT:
            raise ValueError("dfl_weight goes with a distribution box head (regression_bins); this model has none")
        if not float(dfl_weight) >= 0:
            raise ValueError("dfl_weight must be >= 0, got {}".format(dfl_weight))
        self.dfl_weight = float(dfl_weight)
        if self.regression_bins:
            from ..ops import fp8 as _fp8
            if _fp8.enabled():
                raise ValueError("regression_bins={} does not go with fp8: the regression final's {} outputs would run "
                                 "in fp8".format(self.regression_bins, 4 * self.regression_bins * model.num_anchors))
        if classification_loss != "focal" and classification_loss not in losses.CLS_KINDS:
            raise ValueError("classification_loss must be 'focal' or one of {}, got {!r}".format(
                losses.CLS_KINDS, classification_loss))
        if classification_loss != "focal":
            from ..ops import fp8 as _fp8
            if _fp8.enabled():
                raise ValueError("classification_loss={!r} does not go with fp8: the classification final's focal loss "
                                 "is part of the fp8 epilogue".format(classification_loss))
        self.classification_loss = classification_loss
        if getattr(model, "head_norm", None) is not None:
            from ..ops import fp8 as _fp8
            if _fp8.enabled():
                raise ValueError("head_norm={!r} does not go with fp8: the fp8 tower layers hand fp8 copies of their "
                                 "ReLU outputs to each other".format(model.head_norm))
        if assigner not in ("iou", "atss"):
            raise ValueError("assigner must be 'iou' or 'atss', got {!r}".format(assigner))
        if assigner == "iou" and atss_topk != anchor_ops.ATSS_TOPK:
            raise ValueError("atss_topk goes with assigner='atss'; the fixed-threshold rule has no top-k")
        self.assigner = assigner
        self.atss_topk = anchor_ops._check_topk(atss_topk)
        if regression_loss != "smooth_l1" and regression_loss not in losses.IOU_KINDS:
            raise ValueError("regression_loss must be 'smooth_l1' or one of {}, got {!r}".format(
                losses.IOU_KINDS, regression_loss))
        if regression_loss == "smooth_l1" and regression_weight != 1.0:
            raise ValueError("regression_weight goes with the IoU regression losses; smooth_l1 has no weight")
        self.regression_loss = regression_loss
        self.regression_weight = float(regression_weight)
        self.device = device or (runtime.device() if runtime.is_initialized() else torch.device("cpu"))
        self.model = model.to(self.device)
        self.compute_dtype = compute_dtype
        self.flat = FlatParams(backward_order(self.model), device=self.device)
        if optimizer == "adam":
            if momentum or nesterov or weight_decay:
                raise ValueError("momentum, nesterov and weight_decay belong to optimizer='sgd'")
            self.base_optimizer = KerasAdam(self.flat, lr=lr, clipnorm=clipnorm, ema_decay=ema_decay)
        elif optimizer == "sgd":
            self.base_optimizer = KerasSGD(self.flat, lr=lr, momentum=momentum, nesterov=nesterov,
                                           weight_decay=weight_decay, clipnorm=clipnorm, ema_decay=ema_decay)
        else:
            raise ValueError("optimizer must be 'adam' or 'sgd', got {!r}".format(optimizer))
        self.optimizer = DistributedOptimizer(self.base_optimizer, compression=compression or Compression.none,
                                              clip_mode=clip_mode, bucket_bytes=bucket_bytes, overlap=overlap)
        if regression_loss != "smooth_l1":
            # what a snapshot records about the loss (io.checkpoint.training_config reads it off the optimizer)
            self.base_optimizer.regression_loss = regression_loss
            self.base_optimizer.regression_weight = self.regression_weight
        if classification_loss != "focal":
            self.base_optimizer.classification_loss = classification_loss
        if assigner != "iou":
            # likewise the target assignment
            self.base_optimizer.assigner = assigner
            self.base_optimizer.atss_topk = self.atss_topk
        if self.dfl_weight != losses.DFL_WEIGHT:
            self.base_optimizer.dfl_weight = self.dfl_weight
        self.anchors = anchor_ops.AnchorCache()
        self.num_classes = model.num_classes
        self.target_backend = target_backend
        self.stop_training = False
        self.shapes_callback = None
        self.last_logs: Dict[str, torch.Tensor] = {}
        self.compute_weights = None
        self._ema_swapped = False   # inside ema_weights(): flat.data holds the average, the EMA buffer the weights
        from ..ops import native
        # zero-padded gradient rows of the two final layers: one buffer per shape a captured step holds plus a
        # floating one (a graph keeps the pointer it was captured with)
        self._cls_pad_buf = native.ShapeSlots()
        self._focal_req = None      # ops.conv_launch.FocalRequest: the classification final's fused focal loss
        self._reg_pad_buf = native.ShapeSlots()
        self.step_graphs = None     # train.step_graphs.StepGraphs once enable_graphs() ran
        from ..ops import fp8 as _fp8
        _fp8.reset_state()      # process-wide fp8 delayed-scaling state (the packed features) starts per model
        if (self.device.type == "cuda" and compute_dtype == torch.bfloat16 and native.available()
                and hasattr(self.model, "convs") and os.environ.get("MXR_NO_COMPUTE_WEIGHTS") != "1"):
            # bf16 W*s compute copies maintained by the fused Adam kernel (no per-layer fold/cast)
            self.compute_weights = native.ComputeWeights(self.flat, self.model.convs())
            native.set_compute_weights(self.compute_weights)
        if self.device.type == "cuda" and native.available() and os.environ.get("MXR_NO_GRAD_SINKS") != "1":
            # conv weight/bias gradients accumulate straight into flat.grad (no autograd adds)
            native.set_grad_sinks(native.GradSinks(self.flat, self.optimizer.notify_grad_ready))

    # ---------------------------------------------------------------- targets
    def compute_targets(self, images: torch.Tensor, gt: torch.Tensor, gt_count: torch.Tensor, image_hw: torch.Tensor):
        H, W = int(images.shape[1]), int(images.shape[2])
        anchors = self.anchors.get((H, W), self.device, self.shapes_callback)
        centers = self.anchors.centers((H, W), self.device, self.shapes_callback)
        from ..ops import native
        use_hip = (self.target_backend == "hip" or
                   (self.target_backend == "auto" and anchors.is_cuda and native.available()))
        if self.assigner == "atss":
            levels = self.anchors.levels((H, W), self.device, self.shapes_callback)
            if use_hip:
                return native.atss_targets(anchors, levels, gt, gt_count, image_hw, topk=self.atss_topk, centers=centers)
            state, label, reg = anchor_ops.atss_targets_torch(anchors, levels, gt, gt_count, image_hw,
                                                              topk=self.atss_topk, centers=centers)
            return state, label, reg, (state == 1).sum().to(torch.int32).reshape(1)
        if use_hip:
            return native.anchor_targets(anchors, gt, gt_count, image_hw, centers=centers)
        state, label, reg = anchor_ops.anchor_targets_torch(anchors, gt, gt_count, image_hw, centers=centers)
        return state, label, reg, (state == 1).sum().to(torch.int32).reshape(1)

    # ---------------------------------------------------------------- step
    def _fused_losses(self) -> bool:
        from ..ops import native
        return self.device.type == "cuda" and native.available()

    def forward_backward(self, images, gt, gt_count, image_hw):
        """Targets + forward + losses + backward.  Returns (reg_loss, cls_loss) device scalars."""
        with _range("targets"):
            state, label, reg_t, npos = self.compute_targets(images, gt, gt_count, image_hw)
        x = images.to(self.compute_dtype)
        req = self._focal_request(state, label, npos)
        if self.regression_bins and self._fused_losses():
            # the distribution head's integral runs on positive rows only (RetinaNet._with_integral)
            self.model.integral_request = state
        # the losses below read the regression output on state == 1 rows only (smooth_l1_kernel / iou_loss_kernel):
        # the model may run the regression tower's forward where that is (ops.row_activity.FwdChain).  This request is
        # what enforces the contract: the quality losses and the distribution head read more, and get none
        sparse_reg = (self._fused_losses() and self.classification_loss == "focal" and not self.regression_bins
                      and self.regression_loss in ("smooth_l1", "giou", "diou", "ciou"))
        if sparse_reg:
            self.model.positive_request = state
        with _range("forward"):
            try:
                out = self.model(x)
            finally:
                if req is not None:
                    self.model.focal_request = None
                if self.regression_bins:
                    self.model.integral_request = None
                if sparse_reg:
                    self.model.positive_request = None
        with _range("backward"):
            return self._losses_backward(out, reg_t, state, label, npos, self._loss_anchors(images))

    def _loss_anchors(self, images):
        """The anchors of the batch's padded shape for the IoU regression losses (the cache's persistent tensor: a
        captured step keeps a valid pointer) and the IoU-aware classification losses; None with smooth-L1 and focal,
        which need none."""
        if self.regression_loss == "smooth_l1" and self.classification_loss == "focal":
            return None
        return self.anchors.get((int(images.shape[1]), int(images.shape[2])), self.device, self.shapes_callback)

    def _regression_fwd_bwd(self, reg, reg_t, state, npos, anchors, **pad):
        """The fused regression loss kernel of this trainer: (loss, d loss / d reg)."""
        from ..ops import native
        if self.regression_loss == "smooth_l1":
            return native.smooth_l1_fwd_bwd(reg, reg_t, state, npos, **pad)
        return native.iou_loss_fwd_bwd(reg, reg_t, anchors, state, npos, kind=self.regression_loss,
                                       weight=self.regression_weight, **pad)

    def _regression_torch(self, reg, reg_t, state, anchors):
        if self.regression_loss == "smooth_l1":
            return losses.smooth_l1_loss(reg, reg_t, state, backend="torch")
        return losses.iou_loss(reg, reg_t, state, anchors, self.regression_loss, self.regression_weight,
                               backend="torch")

    def _regression_terms_torch(self, out, reg_t, state, anchors):
        """The logged regression loss as torch expressions: the box loss and, with a distribution head, + DFL."""
        loss = self._regression_torch(out["regression"], reg_t, state, anchors)
        if self.regression_bins:
            loss = loss + losses.distribution_focal_loss(out["regression_logits"], reg_t, state, self.regression_bins,
                                                         self.regression_range, self.dfl_weight, backend="torch")
        return loss

    def _dist_losses_fused(self, out, reg_t, state, npos, anchors, A, rsink):
        """The fused losses of a distribution head: the box loss kernel on the integral deltas (plain gradient layout),
        then box_dist.hip: DFL and d(box loss + DFL)/d(logits), into the regression final's zero-padded rows where it
        has them.  Returns (the tensor to backpropagate from, regression loss, its gradient)."""
        from ..ops import native
        from ..ops import fp8 as _fp8
        if _fp8.enabled():      # switched on after the constructor's check
            raise RuntimeError("regression_bins={} does not go with fp8".format(self.regression_bins))
        K, R = self.regression_bins, self.regression_range
        logits, reg = out["regression_logits"], out["regression"]
        if reg.requires_grad:
            # the model ran the differentiable torch integral (a form box_dist.hip does not serve)
            loss = self._regression_terms_torch(out, reg_t, state, anchors)
            return loss, loss, None
        box_loss, dreg = self._regression_fwd_bwd(reg, reg_t, state, npos, anchors)
        W = 4 * K * A
        if rsink is not None and _PAD_FOCAL and logits.dtype == torch.bfloat16 and logits.shape[1] % A == 0 and W % 64:
            key = (logits.shape[0], logits.shape[1] // A, (W + 63) // 64 * 64, logits.device)
            buf = self._reg_pad_buf.get(key, lambda: torch.zeros(key[:3], dtype=logits.dtype, device=logits.device))
            dfl, dpad = native.box_dist_fwd_bwd(logits.detach(), dreg, reg_t, state, npos, K, R, self.dfl_weight,
                                                grad_out=buf, group=A)
            rsink["dy"] = dpad
            dlog = torch.zeros((), dtype=logits.dtype, device=logits.device).expand(logits.shape)
        else:
            # (W % 64 == 0: the plain layout is the final layer's own)
            dfl, dlog = native.box_dist_fwd_bwd(logits.detach(), dreg, reg_t, state, npos, K, R, self.dfl_weight)
        return logits, box_loss + dfl, dlog

    def _check_quality_rows(self, cls, reg, anchors):
        """An IoU-aware classification loss reads row r of the regression output for row r of the logits."""
        if not (cls.dim() == 3 and reg.dim() == 3 and reg.shape[:2] == cls.shape[:2] and reg.shape[2] == 4
                and anchors is not None and anchors.shape[0] == cls.shape[1]):
            raise ValueError("classification_loss={!r} needs the regression output (B, A, 4) in the row order of the "
                             "classification output (B, A, C) and the A anchors of the batch's shape; got {} and {}"
                             .format(self.classification_loss, tuple(reg.shape), tuple(cls.shape)))

    def _classification_fwd_bwd(self, out, reg_t, state, label, npos, anchors, **pad):
        """The fused classification loss kernel of this trainer: (loss, d loss / d logits)."""
        from ..ops import native
        cls = out["classification"]
        if getattr(self.model, "head_norm", None) is not None:
            from ..ops import fp8 as _fp8
            if _fp8.enabled():      # switched on after the constructor's check
                raise RuntimeError("head_norm={!r} does not go with fp8".format(self.model.head_norm))
        if self.classification_loss == "focal":
            return native.focal_fwd_bwd(cls, state, label, npos, **pad)
        from ..ops import fp8 as _fp8
        if _fp8.enabled():      # switched on after the constructor's check
            raise RuntimeError("classification_loss={!r} does not go with fp8".format(self.classification_loss))
        reg = out["regression"].detach()
        self._check_quality_rows(cls, reg, anchors)
        return native.quality_loss_fwd_bwd(cls, reg, reg_t, anchors, state, label, npos,
                                           kind=self.classification_loss, **pad)

    def _classification_torch(self, out, reg_t, state, label, anchors):
        cls = out["classification"]
        if self.classification_loss == "focal":
            return losses.focal_loss(cls, state, label, backend="torch")
        self._check_quality_rows(cls, out["regression"], anchors)
        return losses.quality_loss(cls, out["regression"], reg_t, state, label, anchors, self.classification_loss,
                                   backend="torch")

    def _focal_request(self, state, label, npos):
        """This step's targets for the classification final's fused focal loss (bf16 HIP heads with the padded
        focal gradient), handed to the model for its forward; None where the fusion does not apply (an IoU-aware
        classification loss needs the regression output: the final writes its logits and quality_loss.hip reads them)."""
        if self.classification_loss != "focal":
            return None
        if not (self._fused_losses() and _PAD_FOCAL and self.compute_dtype == torch.bfloat16
                and hasattr(self.model, "cls_pad_sink")):
            return None
        from ..ops.conv_launch import FocalRequest
        if self._focal_req is None:
            self._focal_req = FocalRequest()
        A = self.model.num_anchors if hasattr(self.model, "num_anchors") else 9
        self._focal_req.set(state, label, npos, A)
        self.model.focal_request = self._focal_req
        return self._focal_req

    def _losses_backward(self, out, reg_t, state, label, npos, anchors=None):
        if self._fused_losses():
            # fused loss kernels emit d(loss)/d(outputs) directly; backprop from the outputs
            from ..ops import native
            reg = out["regression"]
            A = self.model.num_anchors if hasattr(self.model, "num_anchors") else 9
            rsink = getattr(self.model, "reg_pad_sink", None)
            if self.regression_bins:
                reg, reg_loss, dreg = self._dist_losses_fused(out, reg_t, state, npos, anchors, A, rsink)
            elif rsink is not None and _PAD_FOCAL and reg.dtype == torch.bfloat16 and reg.shape[1] % A == 0 and \
                    (4 * A) % 64:
                # the loss kernel writes d(loss)/d(regression) into the final layer's 64-padded rows (36 -> 64);
                # the layer's data / weight / bias gradients then read them as is (no pad, cast or slice)
                key = (reg.shape[0], reg.shape[1] // A, (4 * A + 63) // 64 * 64, reg.device)
                buf = self._reg_pad_buf.get(key, lambda: torch.zeros(key[:3], dtype=reg.dtype, device=reg.device))
                reg_loss, dpad = self._regression_fwd_bwd(reg, reg_t, state, npos, anchors, grad_out=buf, group=A)
                rsink["dy"] = dpad
                dreg = torch.zeros((), dtype=reg.dtype, device=reg.device).expand(reg.shape)
            else:
                reg_loss, dreg = self._regression_fwd_bwd(reg, reg_t, state, npos, anchors)
            cls = out["classification"]
            sink = getattr(self.model, "cls_pad_sink", None)
            cp = (A * cls.shape[-1] + 63) // 64 * 64
            req = self._focal_req
            if req is not None and req.loss is not None:
                # the final layer's forward fused the focal loss: its loss and the padded gradient rows (in the
                # pad sink) are already there; the logits were never written
                cls_loss = req.loss
                req.loss = None
                dcls = torch.zeros((), dtype=cls.dtype, device=cls.device).expand(cls.shape)
            elif sink is not None and _PAD_FOCAL and cls.dtype == torch.bfloat16 and cls.shape[1] % A == 0 and \
                    cls.shape[-1] % 8 == 0 and (A * cls.shape[-1]) % 64:
                # the focal kernel writes d(loss)/d(logits) straight into the final layer's zero-padded
                # data-gradient rows; autograd carries a zero-stride placeholder
                key = (cls.shape[0], cls.shape[1] // A, cp, cls.device)
                buf = self._cls_pad_buf.get(key, lambda: torch.zeros(key[:3], dtype=cls.dtype, device=cls.device))
                cls_loss, dpad = self._classification_fwd_bwd(out, reg_t, state, label, npos, anchors, grad_out=buf,
                                                              group=A)
                sink["dy"] = dpad
                dcls = torch.zeros((), dtype=cls.dtype, device=cls.device).expand(cls.shape)
            else:
                cls_loss, dcls = self._classification_fwd_bwd(out, reg_t, state, label, npos, anchors)
            torch.autograd.backward([reg, cls], [dreg, dcls])
        else:
            reg_loss = self._regression_terms_torch(out, reg_t, state, anchors)
            cls_loss = self._classification_torch(out, reg_t, state, label, anchors)
            (reg_loss + cls_loss).backward()
        return reg_loss.detach(), cls_loss.detach()

    def forward_losses(self, images, gt, gt_count, image_hw):
        """Loss values only (no backward) -- used by evaluation/tests."""
        with torch.no_grad():
            state, label, reg_t, npos = self.compute_targets(images, gt, gt_count, image_hw)
            out = self.model(images.to(self.compute_dtype))
            anchors = self._loss_anchors(images)
            reg_loss = self._regression_terms_torch(out, reg_t, state, anchors)
            cls_loss = self._classification_torch(out, reg_t, state, label, anchors)
        return reg_loss, cls_loss

    def train_on_batch(self, images: torch.Tensor, gt: torch.Tensor, gt_count: torch.Tensor,
                       image_hw: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Returns device scalars {loss, regression_loss, classification_loss} (no host sync)."""
        if not self.model.training:
            # (Module.train() walks all ~150 modules: ~0.9 ms of host time, which sat in front of the
            # step's first kernels every step when called unconditionally)
            self.model.train()
        if self._ema_swapped:
            raise RuntimeError("train_on_batch inside ema_weights(): the averaged weights are in place")
        if self.step_graphs is not None:
            return self.step_graphs.step(images, gt, gt_count, image_hw)
        return self._train_on_batch(images, gt, gt_count, image_hw)

    def _train_on_batch(self, images, gt, gt_count, image_hw):
        self.optimizer.zero_grad()
        images = images.to(self.device, non_blocking=True)
        gt = gt.to(self.device, non_blocking=True)
        gt_count = gt_count.to(self.device, non_blocking=True)
        image_hw = image_hw.to(self.device, non_blocking=True)
        reg_loss, cls_loss = self.forward_backward(images, gt, gt_count, image_hw)
        loss = reg_loss + cls_loss
        with _range("optimizer"):
            self.optimizer.step()
        logs = {"loss": loss, "regression_loss": reg_loss, "classification_loss": cls_loss}
        self.last_logs = logs
        return logs

    def graph_step(self, images, gt, gt_count, image_hw, warmup: int = 2):
        """Capture ONE whole training step (targets, forward, losses, backward, clip, Adam, compute-
        weight refresh) in a HIP graph; returns ``replay(images, gt, gt_count, image_hw) -> logs``.

        Inputs are copied into static device buffers (same shapes as the example batch).  Every
        kernel of the step is launched by a single graph launch -- no per-kernel CPU dispatch.

        Multi-rank runs capture the native RCCL bucket engine's work too (``parallel.native_comm``): each
        bucket's readiness event, the in-order ``ncclAllReduce`` on the comm stream and the optimizer's waits on
        the done events become graph nodes, so a replay issues the all-reduces exactly where the eager step
        does, overlapped with the backward.  Every rank captures the same collective sequence and replays it in
        lockstep.  (The torch.distributed engine is not captured: gloo runs on the host.)  One graph per batch
        shape: a caller with several padded shape classes keeps one replay per class.  Not with fp8 (its
        delayed-scaling state advances on the host every step).
        """
        from ..ops import fp8 as _fp8
        if runtime.distributed() and self.optimizer.native is None:
            raise RuntimeError("graph_step across ranks needs the native RCCL bucket engine (MXR_COMM=auto/native); "
                               "the torch.distributed path runs eagerly")
        if _fp8.enabled():
            raise RuntimeError("graph_step: the fp8 delayed-scaling state advances on the host each step")
        if self.step_graphs is not None:
            raise RuntimeError("graph_step: this trainer already replays per-shape-class graphs (enable_graphs)")
        dev = self.device
        static = {"images": images.to(dev).clone(), "gt": gt.to(dev).clone(), "gt_count": gt_count.to(dev).clone(),
                  "image_hw": image_hw.to(dev).clone()}
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.train_on_batch(**static)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        # thread-local capture: the comm engine's watchdog thread may still poll an earlier step's events
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            logs = self.train_on_batch(**static)
        from ..ops import native
        plan = native.adam_plan(self.flat) if native.available() else None

        def replay(images, gt, gt_count, image_hw):
            for k, v in (("images", images), ("gt", gt), ("gt_count", gt_count), ("image_hw", image_hw)):
                if v.data_ptr() != static[k].data_ptr():
                    static[k].copy_(v, non_blocking=True)
            if plan is not None and hasattr(self.base_optimizer, "momentum"):
                plan.set_momentum(self.base_optimizer.momentum)     # outside the graph, like the lr in enable_graphs
            graph.replay()
            # the captured Adam advances the device step counter; keep the host mirrors in sync
            self.base_optimizer.iterations += 1
            if plan is not None:
                plan.host_iter += 1
            return logs

        # capturing RECORDS the step without executing it, but the host-side counters advanced
        # while the Python ran -> undo that advance
        self.base_optimizer.iterations -= 1
        if plan is not None:
            plan.host_iter -= 1
        self._graph = graph
        return replay

    # ---------------------------------------------------------------- per-shape-class step graphs
    def enable_graphs(self, max_shapes: int = 8, eager_sightings: int = 2):
        """Route ``train_on_batch`` through a per-shape-class cache of captured steps (``train.step_graphs``):
        a class's first ``eager_sightings`` batches run eagerly, the next one is captured and from then on replayed;
        at most ``max_shapes`` classes are captured.  Same conditions as :meth:`graph_step`.  Returns the cache."""
        from ..ops import fp8 as _fp8
        from .step_graphs import StepGraphs
        if self.device.type != "cuda":
            raise RuntimeError("enable_graphs: HIP graphs need a GPU device")
        if runtime.distributed() and self.optimizer.native is None:
            raise RuntimeError("enable_graphs across ranks needs the native RCCL bucket engine (MXR_COMM=auto/native); "
                               "the torch.distributed path runs eagerly")
        if _fp8.enabled():
            raise RuntimeError("enable_graphs: the fp8 delayed-scaling state advances on the host each step")
        self.step_graphs = StepGraphs(self, max_shapes=max_shapes, eager_sightings=eager_sightings)
        return self.step_graphs

    def adam_plan(self):
        """The fused optimizer kernel's device tables and host mirrors -- Adam and SGD share them -- (None where the
        torch expression runs)."""
        from ..ops import native
        return native.adam_plan(self.flat) if self.base_optimizer._use_hip() else None

    def persistent_slots(self):
        """Every per-shape persistent buffer a captured step may hold a pointer to."""
        slots = [self._cls_pad_buf, self._reg_pad_buf]
        if self._focal_req is not None:
            slots += [self._focal_req._buf, self._focal_req._qbuf]
        return slots

    # ---------------------------------------------------------------- keras-ish
    @property
    def lr(self) -> float:
        return self.base_optimizer.lr

    @lr.setter
    def lr(self, v: float) -> None:
        self.base_optimizer.lr = float(v)

    @property
    def momentum(self) -> float:
        """The base optimizer's momentum (SGD); an AttributeError with Adam, which has none."""
        return self.base_optimizer.momentum

    @momentum.setter
    def momentum(self, v: float) -> None:
        if not hasattr(self.base_optimizer, "momentum"):
            raise AttributeError("the {} optimizer has no momentum".format(self.base_optimizer.class_name))
        self.base_optimizer.momentum = float(v)

    def state_for_broadcast(self):
        return [self.flat.data] + [b for b in self.model.buffers()]

    def on_weights_changed(self) -> None:
        """Call after weights/optimizer state were replaced (broadcast, checkpoint restore)."""
        if self.step_graphs is not None:
            self.step_graphs.invalidate()       # the flat buffers are rebound and the compute copies rebuilt
        self.flat.rebind()
        if self.base_optimizer.ema is not None and self.base_optimizer.ema_updates == 0:
            # a run that has not averaged yet (--weights / --imagenet-weights / broadcast): the average starts from
            # the weights as they are now; a restored average is left alone
            self.base_optimizer.seed_ema()
        if self.compute_weights is not None:
            self.compute_weights.build()     # BN scales may have changed too

    # ---------------------------------------------------------------- weight EMA
    def _swap_ema(self) -> None:
        opt = self.base_optimizer
        if opt._use_hip():
            from ..ops import native
            native.swap_refresh(self.flat, opt.ema)     # one pass: exchange + the bf16 compute copies
        else:
            tmp = self.flat.data.clone()
            self.flat.data.copy_(opt.ema)
            opt.ema.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the body on the averaged weights (evaluation): on entry the weights and their moving average are
        exchanged in place, on exit exchanged back.  No pointer moves, so captured step graphs stay valid and
        ``on_weights_changed`` is not called.  Only the trainable parameters are averaged; everything else (frozen
        BN statistics, live BN buffers) is what it is.  Not reentrant, and no training step inside."""
        if self.base_optimizer.ema is None:
            raise RuntimeError("ema_weights: this trainer keeps no weight EMA (ema_decay=0)")
        if self._ema_swapped:
            raise RuntimeError("ema_weights: already inside (the averaged weights are in place)")
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._ema_swapped = False
