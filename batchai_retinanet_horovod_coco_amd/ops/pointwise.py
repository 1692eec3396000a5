"""Pointwise (1x1) convolution of MobileNet's ``conv_pw_*`` layers on NHWC activations: no bias, no activation (a
batch-norm follows).

:func:`pointwise_conv_torch` is the torch expression -- ``F.conv2d`` on the NCHW view, back to NHWC: the CPU path, the
fallback for what ``csrc/kernels/pwconv.hip`` does not serve and, in float64, the oracle of its tests.
:func:`pointwise_conv` dispatches to the kernels (``native.PointwiseConvFn``) on the GPU.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn.functional as F

_FALLBACK_WARNED = set()


def pointwise_conv_torch(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """The torch expression: ``x`` NHWC, ``weight`` ``(Co, Ci, 1, 1)``; returns NHWC (a view of the NCHW result)."""
    return F.conv2d(x.permute(0, 3, 1, 2), weight.to(x.dtype)).permute(0, 2, 3, 1)


def takes_native(x: torch.Tensor, co: int, backend: str = "auto") -> bool:
    """Whether :func:`pointwise_conv` would run the kernels on this NHWC input."""
    if backend == "torch":
        return False
    from . import native
    return x.is_cuda and native.available() and native.pwconv_served(x, co, auto=backend != "native")


def pointwise_conv(x: torch.Tensor, weight: torch.Tensor, backend: str = "auto") -> torch.Tensor:
    """HIP 1x1 conv on NHWC ``x`` where the kernels serve it, else the torch expression.

    ``backend="torch"`` forces the torch expression; ``backend="native"`` raises where the kernels do not serve."""
    if backend not in ("auto", "native", "torch"):
        raise ValueError("pointwise_conv: backend 'auto', 'native' or 'torch' expected, got {!r}".format(backend))
    if backend != "torch":
        from . import native
        if backend == "auto" and (int(x.shape[-1]), int(weight.shape[0])) in native.PW_AUTO_EXCLUDED:
            pass        # a measured choice, not a missing kernel: no warning
        elif x.is_cuda and native.available():
            try:
                return native.PointwiseConvFn.apply(x, weight)
            except native.NotServed:
                if backend == "native":
                    raise
                key = (int(x.shape[-1]), int(weight.shape[0]), x.dtype)
                if key not in _FALLBACK_WARNED:
                    # once per form: a production layer on the NCHW-view conv2d should be noticed
                    _FALLBACK_WARNED.add(key)
                    warnings.warn("pwconv.hip does not serve Ci = {}, Co = {}, {}: the pointwise conv runs as the "
                                  "torch expression".format(*key))
        elif backend == "native":
            raise RuntimeError("pointwise_conv: backend 'native' needs a GPU tensor and the HIP kernel library")
    return pointwise_conv_torch(x, weight)
