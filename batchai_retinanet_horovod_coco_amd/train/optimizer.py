"""Keras-semantics Adam and SGD with ``clipnorm`` over flat fp32 buffers.

Spec: ``keras.optimizers.adam(lr=1e-5, clipnorm=0.001)`` at ``/root/reference/train.py:104``
(SURVEY §2.8.7):

    g <- g * clipnorm / ||g||   if ||g|| >= clipnorm   (global L2 norm over ALL grads)
    t  = iterations + 1
    lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
    m  = beta1 m + (1 - beta1) g
    v  = beta2 v + (1 - beta2) g^2
    p -= lr_t * m / (sqrt(v) + eps)          eps = K.epsilon() = 1e-7 (outside the bias fix)

The update runs as ONE fused multi-tensor HIP kernel over the flat buffers on the GPU
(``csrc/kernels/optim.hip``: gradient pre-scale (1/world, clip factor) + Adam + refresh of
the bf16 compute weights), and as the equivalent torch expression on the CPU.  The clip
factor and lr_t live on the device so a step never synchronises with the host.

:class:`KerasSGD` (Keras 2 ``SGD(lr, momentum, decay, nesterov)`` plus coupled weight decay) shares the norm, the
clip factor and the backend choice with it (:class:`_FlatOptimizer`) and runs as one fused launch too
(``mxr_sgd_step``).

Both take ``ema_decay = D`` (0 < D < 1; 0, the default, is off): an fp32 exponential moving average of the flat
weights, seeded with a copy of them and updated after every step, ``ema = d_n * ema + (1 - d_n) * p_new`` with
``d_n = min(D, (1 + n) / (10 + n))`` in fp32 and ``n = iterations + 1 - ema_start`` the 1-based index of the update.
On the GPU the EMA forms of the same fused launches carry it (``mxr_adam_step_ema`` / ``mxr_sgd_step_ema``; the decay
is derived on the device from the step counter, so a replayed graph sees a new one each step).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .flat import FlatParams


class _FlatOptimizer:
    """What every optimizer over the flat buffers shares: the global gradient norm, the ``clipnorm`` factor, the
    choice between the fused HIP kernels and the torch expression, and Keras' ``decay`` schedule.  A subclass sets
    ``class_name`` (the Keras class the checkpoints record) and implements ``apply`` / ``state_tensors`` /
    ``get_config``."""

    class_name = ""

    def __init__(self, flat: FlatParams, lr: float, decay: float, clipnorm: Optional[float], backend: str,
                 ema_decay: float = 0.0):
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError("ema_decay must be in [0, 1), got {!r}".format(ema_decay))
        self.flat = flat
        self.lr = float(lr)
        self.initial_lr = float(lr)
        self.decay = decay
        self.clipnorm = clipnorm
        self.iterations = 0                       # host mirror (the step count is deterministic)
        self.backend = backend
        self._dev = flat.data.device
        # exponential moving average of the weights, carried by the same fused launch (0: off, no buffer)
        self.ema_decay = float(ema_decay)
        self.ema_start = 0                        # ``iterations`` when the average was seeded
        self.ema = flat.data.detach().clone() if self.ema_decay > 0 else None

    # -------------------------------------------------------------- weight EMA
    @property
    def ema_updates(self) -> int:
        """EMA updates so far: derived from the step count, there is no counter of its own."""
        return self.iterations - self.ema_start

    def ema_decay_at(self, n: int) -> float:
        """``d_n = min(D, (1 + n) / (10 + n))`` of the ``n``-th EMA update (1-based), in fp32 arithmetic: TensorFlow's
        ``ExponentialMovingAverage(num_updates)`` ramp, which the fused kernels' prologue evaluates on the device."""
        import numpy as np
        d = np.float32(1 + n) / np.float32(10 + n)
        return float(min(np.float32(self.ema_decay), d))

    def seed_ema(self) -> None:
        """Start the average over: a copy of the weights as they are, no update counted."""
        if self.ema is not None:
            self.ema.copy_(self.flat.data)
            self.ema_start = self.iterations

    def _ema_torch(self) -> None:
        """The torch expression of the EMA update that follows this step's weight update (``iterations`` not yet
        advanced)."""
        if self.ema is not None:
            d = self.ema_decay_at(self.iterations + 1 - self.ema_start)
            self.ema.mul_(d).add_(self.flat.data, alpha=1.0 - d)

    def _ema_config(self) -> Dict:
        return {"ema_decay": self.ema_decay} if self.ema is not None else {}

    def _ema_state(self) -> Dict:
        return {"ema": self.ema} if self.ema is not None else {}

    def _ema_args(self) -> Dict:
        """What the fused step takes for the EMA form (empty: the plain entry point)."""
        if self.ema is None:
            return {}
        return {"ema": self.ema, "ema_decay": self.ema_decay, "ema_start": self.ema_start}

    def _use_hip(self) -> bool:
        from ..ops import native
        if self.backend == "torch":
            return False
        return self.flat.data.is_cuda and native.available()

    # -------------------------------------------------------------- math
    def grad_norm(self, grad: Optional[torch.Tensor] = None) -> torch.Tensor:
        g = self.flat.grad if grad is None else grad
        if self._use_hip():
            from ..ops import native
            return native.l2norm(g)
        return torch.linalg.vector_norm(g.float())

    def norm_and_scale(self, norm_mul: float = 1.0, scale_mul: float = 1.0):
        """(norm * norm_mul, clip_factor(norm * norm_mul) * scale_mul) as 0-d device tensors; on the HIP
        path ONE fused reduction + finalize launch instead of the norm and five scalar torch ops."""
        if self._use_hip():
            from ..ops import native
            out = native.grad_norm_clip(self.flat.grad, norm_mul, float(self.clipnorm or 0.0), scale_mul)
            return out[0], out[1]
        norm = self.grad_norm() * norm_mul
        return norm, self.clip_factor(norm) * scale_mul

    def clip_factor(self, norm: torch.Tensor) -> torch.Tensor:
        if not self.clipnorm or self.clipnorm <= 0:
            return torch.ones((), device=norm.device)
        c = self.clipnorm
        return torch.where(norm >= c, c / norm.clamp_min(1e-30), torch.ones_like(norm))

    def base_lr(self, t: int) -> float:
        """The learning rate of iteration ``t`` (1-based) before any bias correction, ``decay`` included: what the
        fused kernel is handed, by the eager step and -- outside the graph -- before every graph replay."""
        lr = self.lr
        if self.decay > 0:
            lr = lr * (1.0 / (1.0 + self.decay * (t - 1)))
        return lr

    def step(self, world_size: int = 1) -> torch.Tensor:
        """Local step (no communication): clip, then the update.  Returns the pre-clip norm."""
        norm, scale = self.norm_and_scale(1.0, 1.0 / world_size)
        self.apply(scale)
        return norm

    def zero_grad(self) -> None:
        self.flat.zero_grad()


class KerasAdam(_FlatOptimizer):
    class_name = "Adam"

    def __init__(self, flat: FlatParams, lr: float = 1e-5, beta_1: float = 0.9, beta_2: float = 0.999,
                 epsilon: float = 1e-7, decay: float = 0.0, clipnorm: Optional[float] = 0.001,
                 amsgrad: bool = False, backend: str = "auto", ema_decay: float = 0.0):
        if amsgrad:
            raise NotImplementedError("amsgrad is off in the reference optimizer")
        super().__init__(flat, lr, decay, clipnorm, backend, ema_decay)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.m = torch.zeros_like(flat.data)
        self.v = torch.zeros_like(flat.data)

    # -------------------------------------------------------------- keras-ish API
    def get_config(self) -> Dict:
        return dict({"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "decay": self.decay,
                     "epsilon": self.epsilon, "amsgrad": False, "clipnorm": self.clipnorm}, **self._ema_config())

    def state_tensors(self):
        return dict({"m": self.m, "v": self.v}, **self._ema_state())

    def lr_t(self, t: int) -> float:
        lr = self.base_lr(t)
        return lr * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def apply(self, grad_scale: torch.Tensor) -> None:
        """Adam step with ``g_eff = grad * grad_scale`` (grad_scale: 0-d device tensor)."""
        t = self.iterations + 1
        lr_t = self.lr_t(t)
        if self._use_hip():
            from ..ops import native
            native.adam_step(self.flat, self.m, self.v, grad_scale, self.base_lr(t), self.iterations, self.beta_1, self.beta_2,
                             self.epsilon, **self._ema_args())
        else:
            g = self.flat.grad * grad_scale
            self.m.mul_(self.beta_1).add_(g, alpha=1 - self.beta_1)
            self.v.mul_(self.beta_2).addcmul_(g, g, value=1 - self.beta_2)
            self.flat.data.addcdiv_(self.m, self.v.sqrt().add_(self.epsilon), value=-lr_t)
            self._ema_torch()
        self.iterations = t


class KerasSGD(_FlatOptimizer):
    """Keras 2 ``SGD(lr, momentum, decay, nesterov)`` plus coupled L2 weight decay on the parameters of rank >= 2
    (conv kernels; biases and every rank-1 parameter get none):

        lr_t  = lr / (1 + decay * (t - 1))
        g_eff = grad * grad_scale + wd_seg * p
        v     = momentum * v - lr_t * g_eff
        p     = p + v                        (nesterov: p + momentum * v - lr_t * g_eff)

    The clip norm is taken over the raw gradients.  One fused HIP launch over the flat buffers on the GPU
    (``mxr_sgd_step``), which also refreshes the bf16 compute copies; the torch expression elsewhere."""

    class_name = "SGD"

    def __init__(self, flat: FlatParams, lr: float = 0.01, momentum: float = 0.0, decay: float = 0.0,
                 nesterov: bool = False, weight_decay: float = 0.0, clipnorm: Optional[float] = None,
                 backend: str = "auto", ema_decay: float = 0.0):
        if momentum < 0 or weight_decay < 0:
            raise ValueError("momentum and weight_decay must be >= 0")
        super().__init__(flat, lr, decay, clipnorm, backend, ema_decay)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        self.weight_decay = float(weight_decay)
        self.velocity = torch.zeros_like(flat.data)
        self._seg_wd = None         # (weight_decay it was built for, per-segment device table)
        self._wd_flat = None        # the same per element, for the torch expression
        if flat.data.is_cuda:
            self.seg_wd()           # built now: a captured step must not meet its first upload

    def get_config(self) -> Dict:
        return dict({"lr": self.lr, "momentum": self.momentum, "decay": self.decay, "nesterov": self.nesterov,
                     "clipnorm": self.clipnorm, "weight_decay": self.weight_decay}, **self._ema_config())

    def state_tensors(self):
        return dict({"velocity": self.velocity}, **self._ema_state())

    def segment_decay(self):
        """``weight_decay`` for the segments of rank >= 2, 0 for the others: one value per segment."""
        return [self.weight_decay if len(s.shape) >= 2 else 0.0 for s in self.flat.segments]

    def seg_wd(self) -> Optional[torch.Tensor]:
        """The kernel's per-segment decay table (persistent: a captured step holds its pointer), None without decay."""
        if self.weight_decay == 0.0:
            return None
        if self._seg_wd is None or self._seg_wd[0] != self.weight_decay:
            self._seg_wd = (self.weight_decay,
                            torch.tensor(self.segment_decay(), dtype=torch.float32, device=self.flat.data.device))
        return self._seg_wd[1]

    def _decay_per_element(self) -> torch.Tensor:
        if self._wd_flat is None or self._wd_flat[0] != self.weight_decay:
            w = torch.zeros_like(self.flat.data)
            for s, d in zip(self.flat.segments, self.segment_decay()):
                w[s.offset:s.offset + s.numel] = d
            self._wd_flat = (self.weight_decay, w)
        return self._wd_flat[1]

    def apply(self, grad_scale: torch.Tensor) -> None:
        """SGD step with ``g_eff = grad * grad_scale + wd * p`` (grad_scale: 0-d device tensor)."""
        t = self.iterations + 1
        lr_t = self.base_lr(t)
        if self._use_hip():
            from ..ops import native
            native.sgd_step(self.flat, self.velocity, grad_scale, lr_t, self.momentum, self.iterations, self.nesterov,
                            self.seg_wd(), **self._ema_args())
        else:
            g = self.flat.grad * grad_scale
            if self.weight_decay != 0.0:
                g = g + self._decay_per_element() * self.flat.data
            self.velocity.mul_(self.momentum).add_(g, alpha=-lr_t)
            if self.nesterov:
                self.flat.data.add_(self.velocity, alpha=self.momentum).add_(g, alpha=-lr_t)
            else:
                self.flat.data.add_(self.velocity)
            self._ema_torch()
        self.iterations = t
