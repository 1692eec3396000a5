"""Depthwise 3x3 convolution of MobileNet's ``conv_dw_*`` layers on NHWC activations.

Padding follows the Keras model: stride 1 pads one pixel on every side (``Ho = H``), stride 2 pads one pixel at the
bottom and right only and takes a valid window (``Ho = (H - 2) // 2 + 1``).  :func:`depthwise_conv3x3_torch` is the
torch expression -- pad, ``F.conv2d(groups=C)`` on the NCHW view, back to NHWC: the CPU path, the fallback for what
``csrc/kernels/dwconv.hip`` does not serve and, in float64, the oracle of its tests.  :func:`depthwise_conv3x3`
dispatches to the kernels (``native.DepthwiseConv3x3Fn``) on the GPU.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn.functional as F

_FALLBACK_WARNED = set()


def keras_pad(stride: int):
    """``F.pad`` argument (left, right, top, bottom) of a depthwise layer."""
    if stride == 1:
        return (1, 1, 1, 1)
    if stride == 2:
        return (0, 1, 0, 1)
    raise ValueError("depthwise_conv3x3: stride 1 or 2 expected, got {}".format(stride))


def depthwise_conv3x3_torch(x: torch.Tensor, weight: torch.Tensor, stride: int) -> torch.Tensor:
    """The torch expression: ``x`` NHWC, ``weight`` ``(C, 1, 3, 3)``; returns NHWC (a view of the NCHW result)."""
    C = x.shape[3]
    y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), keras_pad(stride)), weight.to(x.dtype), None, stride, 0, 1, C)
    return y.permute(0, 2, 3, 1)


def takes_native(x: torch.Tensor, stride: int, backend: str = "auto") -> bool:
    """Whether :func:`depthwise_conv3x3` would run the kernels on this NHWC input."""
    if backend == "torch":
        return False
    from . import native
    return x.is_cuda and native.available() and native.dwconv_served(x, stride)


def depthwise_conv3x3(x: torch.Tensor, weight: torch.Tensor, stride: int, backend: str = "auto") -> torch.Tensor:
    """HIP depthwise 3x3 conv on NHWC ``x`` where the kernels serve it, else the torch expression.

    ``backend="torch"`` forces the torch expression; ``backend="native"`` raises where the kernels do not serve."""
    if backend not in ("auto", "native", "torch"):
        raise ValueError("depthwise_conv3x3: backend 'auto', 'native' or 'torch' expected, got {!r}".format(backend))
    if backend != "torch":
        from . import native
        if x.is_cuda and native.available():
            try:
                return native.DepthwiseConv3x3Fn.apply(x, weight, int(stride))
            except native.NotServed:
                if backend == "native":
                    raise
                key = (int(x.shape[-1]), int(stride), x.dtype)
                if key not in _FALLBACK_WARNED:
                    # once per form: a production layer on pad + NCHW-view conv2d should be noticed
                    _FALLBACK_WARNED.add(key)
                    warnings.warn("dwconv.hip does not serve C = {}, stride {}, {}: the depthwise conv runs as the "
                                  "torch expression".format(*key))
        elif backend == "native":
            raise RuntimeError("depthwise_conv3x3: backend 'native' needs a GPU tensor and the HIP kernel library")
    return depthwise_conv3x3_torch(x, weight, stride)
