"""One depthwise-separable block of MobileNet in eval mode on NHWC activations:

    ``y = relu6(bn2(conv_pw(relu6(bn1(conv_dw(x))))))``

with Keras' padding of the depthwise 3x3 (stride 1: one pixel on every side; stride 2: bottom and right only, valid
window) and both norms on their running statistics.

:func:`separable_block_eval_torch` is the torch expression: the CPU path, the fallback for what
``csrc/kernels/sepblock.hip`` does not serve and, in float64, the oracle of its tests.  :func:`separable_block_eval`
dispatches to the kernel (``native.sepblock_fwd``: the whole block in one launch, forward only) on the GPU.  The kernel
has two forms that compute the same function, and ``native.sepblock_form(Ci, Co)`` picks between them: the resident
form of ``sepblock.hip`` (``Z`` of a tile in LDS) and, for ``Ci > 256`` with ``Co >= 256``, the K-streamed form of
``csrc/kernels/sepblock_stream.hip``.  There is no switch for the form here.
"""
from __future__ import annotations

import warnings
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

_FALLBACK_WARNED = set()


def separable_block_eval_torch(x: torch.Tensor, dw_weight: torch.Tensor, dw_bn: nn.BatchNorm2d,
                               pw_weight: torch.Tensor, pw_bn: nn.BatchNorm2d, stride: int) -> torch.Tensor:
    """The torch expression: ``x`` NHWC, ``dw_weight`` ``(Ci, 1, 3, 3)``, ``pw_weight`` ``(Co, Ci, 1, 1)``, the two
    ``nn.BatchNorm2d`` modules; returns NHWC (a view of the NCHW result)."""
    z = x.permute(0, 3, 1, 2)
    z = F.pad(z, (1, 1, 1, 1)) if stride == 1 else F.pad(z, (0, 1, 0, 1))
    z = F.relu6(dw_bn(F.conv2d(z, dw_weight.to(x.dtype), stride=stride, groups=x.shape[3])))
    return F.relu6(pw_bn(F.conv2d(z, pw_weight.to(x.dtype)))).permute(0, 2, 3, 1)


def _declined(x, dw_weight, dw_bn, pw_weight, pw_bn) -> Optional[str]:
    """Why the kernel, which is forward only and folds running statistics, may not run on these operands."""
    if dw_bn.training or pw_bn.training:
        return "a batch-norm in training mode takes batch statistics"
    if not dw_bn.track_running_stats or not pw_bn.track_running_stats or not dw_bn.affine or not pw_bn.affine:
        return "a batch-norm without running statistics or without gamma and beta"
    if torch.is_grad_enabled():
        ops = (x, dw_weight, pw_weight, dw_bn.weight, dw_bn.bias, pw_bn.weight, pw_bn.bias)
        if any(t.requires_grad for t in ops):
            return "an operand requires a gradient and the kernel has no backward"
    return None


def takes_native(x: torch.Tensor, dw_weight: torch.Tensor, dw_bn: nn.BatchNorm2d, pw_weight: torch.Tensor,
                 pw_bn: nn.BatchNorm2d, stride: int, backend: str = "auto") -> bool:
    """Whether :func:`separable_block_eval` would run the kernel on this NHWC input."""
    if backend == "torch" or _declined(x, dw_weight, dw_bn, pw_weight, pw_bn) is not None:
        return False
    from . import native
    return (x.is_cuda and native.available()
            and native.sepblock_served(x, dw_weight.shape[0], pw_weight.shape[0], stride, auto=backend != "native"))


def _bn_operands(bn):
    return (bn.weight.float(), bn.bias.float(), bn.running_mean.float(), bn.running_var.float(), float(bn.eps))


def separable_block_eval(x: torch.Tensor, dw_weight: torch.Tensor, dw_bn: nn.BatchNorm2d, pw_weight: torch.Tensor,
                         pw_bn: nn.BatchNorm2d, stride: int, backend: str = "auto") -> torch.Tensor:
    """The block in one HIP launch on NHWC ``x`` where the kernel serves it, else the torch expression.

    ``backend="torch"`` forces the torch expression; ``backend="native"`` raises where the kernel does not serve or may
    not run (a norm in training mode, an operand that requires a gradient while gradients are enabled)."""
    if backend not in ("auto", "native", "torch"):
        raise ValueError("separable_block_eval: backend 'auto', 'native' or 'torch' expected, got {!r}".format(backend))
    if backend != "torch":
        from . import native
        why = _declined(x, dw_weight, dw_bn, pw_weight, pw_bn)
        ci, co = int(dw_weight.shape[0]), int(pw_weight.shape[0])
        if why is not None:
            if backend == "native":
                raise RuntimeError("separable_block_eval: backend 'native' cannot run here: " + why)
        elif backend == "auto" and (ci, co, int(stride)) in native.SEP_AUTO_EXCLUDED:
            pass        # a measured choice, not a missing kernel: no warning
        elif x.is_cuda and native.available():
            try:
                if not native.sepblock_served(x, ci, co, stride):
                    raise native.NotServed("sepblock_fwd")      # before the tap table and the bf16 weight exist
                return native.sepblock_fwd(x, native.dwconv_taps(dw_weight), _bn_operands(dw_bn),
                                           native.pwconv_weight(pw_weight), _bn_operands(pw_bn), stride)
            except native.NotServed:
                if backend == "native":
                    raise
                key = (ci, co, int(stride), x.dtype)
                if key not in _FALLBACK_WARNED:
                    # once per form: a production block on the torch expression should be noticed
                    _FALLBACK_WARNED.add(key)
                    warnings.warn("sepblock.hip does not serve Ci = {}, Co = {}, stride {}, {}: the block runs as the "
                                  "torch expression".format(*key))
        elif backend == "native":
            raise RuntimeError("separable_block_eval: backend 'native' needs a GPU tensor and the HIP kernel library")
    return separable_block_eval_torch(x, dw_weight, dw_bn, pw_weight, pw_bn, stride)
