"""MobileNet's stem convolution (``conv1``: 3x3, stride 2, 3 input channels) on the NHWC image: the Keras padding (one
zero row below, one zero column on the right) and a valid window; no bias, no activation (a batch-norm follows).

:func:`stem_conv3x3_torch` is the torch expression -- pad, ``F.conv2d`` on the NCHW view, back to NHWC: the CPU path,
the fallback for what ``csrc/kernels/stem3x3.hip`` does not serve and, in float64, the oracle of its tests.
:func:`stem_conv3x3` dispatches to the kernels (``native.Stem3x3Fn``) on the GPU.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn.functional as F

_FALLBACK_WARNED = set()


def stem_conv3x3_torch(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """The torch expression: ``x`` NHWC, ``weight`` ``(Co, 3, 3, 3)``; returns NHWC (a view of the NCHW result)."""
    return F.conv2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)), weight.to(x.dtype), stride=2).permute(0, 2, 3, 1)


def takes_native(x: torch.Tensor, co: int, backend: str = "auto") -> bool:
    """Whether :func:`stem_conv3x3` would run the kernels on this NHWC image."""
    if backend == "torch":
        return False
    from . import native
    return x.is_cuda and native.available() and native.stem3_served(x, co, auto=backend != "native")


def stem_conv3x3(x: torch.Tensor, weight: torch.Tensor, backend: str = "auto") -> torch.Tensor:
    """HIP stem conv on NHWC ``x`` where the kernels serve it, else the torch expression.

    ``backend="torch"`` forces the torch expression; ``backend="native"`` raises where the kernels do not serve."""
    if backend not in ("auto", "native", "torch"):
        raise ValueError("stem_conv3x3: backend 'auto', 'native' or 'torch' expected, got {!r}".format(backend))
    if backend != "torch":
        from . import native
        if backend == "auto" and int(weight.shape[0]) in native.STEM3_AUTO_EXCLUDED:
            pass        # a measured choice, not a missing kernel: no warning
        elif x.is_cuda and native.available():
            try:
                return native.Stem3x3Fn.apply(x, weight)
            except native.NotServed:
                if backend == "native":
                    raise
                key = (tuple(x.shape[1:]), int(weight.shape[0]), x.dtype, x.requires_grad)
                if key not in _FALLBACK_WARNED:
                    # once per form: a production stem on the padded NCHW conv2d should be noticed
                    _FALLBACK_WARNED.add(key)
                    warnings.warn("stem3x3.hip does not serve H x W x C = {}, Co = {}, {}, image gradient {}: the stem "
                                  "conv runs as the torch expression".format(*key))
        elif backend == "native":
            raise RuntimeError("stem_conv3x3: backend 'native' needs a GPU tensor and the HIP kernel library")
    return stem_conv3x3_torch(x, weight)
