"""GroupNorm + ReLU of the head towers (``--head-norm gn``), and BatchNorm + activation of the MobileNet backbone.

Statistics are per (image, pyramid level, group) over the level's pixels and the group's channels -- exactly
``F.group_norm`` on the level's own ``[B, C, h, w]`` tensor; gamma and beta are shared by the levels like the conv
weights.  :func:`group_norm_relu_packed` is the torch expression on the packed ``[B, P, C]`` pyramid: the CPU path,
the fallback for what ``csrc/kernels/group_norm.hip`` does not serve and, in float64, the oracle of its tests.
:func:`group_norm_relu` dispatches to the fused kernels (``native.GroupNormReluPackedFn``) on the GPU.

BatchNorm + none / ReLU / ReLU6 on NHWC activations: batch statistics per channel over all pixels of the batch in
training (running statistics updated in place, as ``nn.BatchNorm2d`` does), running statistics in inference.
:func:`batch_norm_act_torch` is the torch expression -- ``F.batch_norm`` on the NCHW view, then the activation: the
CPU path, the fallback for what ``csrc/kernels/batch_norm.hip`` does not serve and, in float64, the oracle of its
tests.  :func:`batch_norm_act` dispatches to the kernels (``native.BatchNormActFn``) on the GPU.
"""
from __future__ import annotations

import warnings
from typing import Sequence, Tuple

import torch
import torch.nn.functional as F

GN_EPS = 1e-5
_FALLBACK_WARNED = set()


def _compute_dtype(t: torch.Tensor) -> torch.dtype:
    return torch.float32 if t.dtype in (torch.bfloat16, torch.float16) else t.dtype


def group_norm_relu_nhwc(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                         eps: float = GN_EPS) -> torch.Tensor:
    """``relu(F.group_norm(x))`` of one level ``[B, h, w, C]`` (arithmetic in fp32 for 16-bit activations)."""
    dt = _compute_dtype(x)
    # a contiguous [B, C, h, w] copy: on the permuted (channels-last) view torch's CPU kernel takes the variance as
    # E[x^2] - mean^2, which loses its digits in fp32 when a group's mean is many standard deviations from zero
    y = F.group_norm(x.permute(0, 3, 1, 2).to(dt).contiguous(), groups, gamma.to(dt), beta.to(dt), eps)
    return torch.relu(y).permute(0, 2, 3, 1).to(x.dtype)


def group_norm_relu_packed(x: torch.Tensor, shapes: Sequence[Tuple[int, int]], gamma: torch.Tensor,
                           beta: torch.Tensor, groups: int, eps: float = GN_EPS) -> torch.Tensor:
    """The torch expression on packed levels: ``x`` is ``[B, P, C]`` with ``P = sum(h * w)`` in level order."""
    B, P, C = x.shape
    if P != sum(h * w for h, w in shapes):
        raise ValueError("group_norm_relu_packed: {} rows do not match the levels {}".format(P, tuple(shapes)))
    out, off = [], 0
    for h, w in shapes:
        lv = x[:, off:off + h * w].reshape(B, h, w, C)
        out.append(group_norm_relu_nhwc(lv, gamma, beta, groups, eps).reshape(B, h * w, C))
        off += h * w
    return torch.cat(out, dim=1)


def group_norm_relu(x: torch.Tensor, shapes: Sequence[Tuple[int, int]], gamma: torch.Tensor, beta: torch.Tensor,
                    groups: int, eps: float = GN_EPS) -> torch.Tensor:
    """Fused HIP GroupNorm + ReLU on the packed pyramid where the kernels serve it, else the torch expression."""
    from . import native
    if x.is_cuda and native.available():
        try:
            return native.GroupNormReluPackedFn.apply(x, gamma, beta, tuple(shapes), int(groups), float(eps))
        except native.NotServed:
            key = (int(x.shape[-1]), int(groups), len(shapes), x.dtype)
            if key not in _FALLBACK_WARNED:
                # once per form: a production shape on five permuted F.group_norm calls per layer should be noticed
                _FALLBACK_WARNED.add(key)
                warnings.warn("group_norm.hip does not serve C = {}, {} groups, {} levels, {}: GroupNorm + ReLU runs as "
                              "the torch expression per level".format(*key))
    return group_norm_relu_packed(x, shapes, gamma, beta, groups, eps)


def _bn_tensors(bn, momentum, eps):
    """(gamma, beta, running_mean, running_var, momentum, eps) of a batch-norm module or of such a 4-tuple."""
    if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
        return bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps
    gamma, beta, running_mean, running_var = bn
    return gamma, beta, running_mean, running_var, momentum, eps


def batch_norm_act_torch(x: torch.Tensor, bn, training: bool, act: str = "relu6", momentum: float = 0.01,
                         eps: float = 1e-3) -> torch.Tensor:
    """The torch expression: ``x`` NHWC, ``bn`` a batch-norm module or ``(gamma, beta, running_mean, running_var)``
    (then ``momentum`` and ``eps`` apply); returns NHWC (a view of the NCHW result).  In training the running
    statistics are updated in place."""
    if act not in ("none", "relu", "relu6"):
        raise ValueError("batch_norm_act: act 'none', 'relu' or 'relu6' expected, got {!r}".format(act))
    gamma, beta, rmean, rvar, momentum, eps = _bn_tensors(bn, momentum, eps)
    if x.dtype not in (torch.bfloat16, torch.float16):
        gamma, beta = gamma.to(x.dtype), beta.to(x.dtype)
    y = F.batch_norm(x.permute(0, 3, 1, 2), rmean, rvar, gamma, beta, bool(training), momentum, eps)
    if act != "none":
        y = F.relu6(y) if act == "relu6" else F.relu(y)
    return y.permute(0, 2, 3, 1)


def bn_takes_native(x: torch.Tensor, training: bool, backend: str = "auto") -> bool:
    """Whether :func:`batch_norm_act` would run the kernels on this NHWC input."""
    if backend == "torch":
        return False
    from . import native
    return x.is_cuda and native.available() and native.bn_served(x, training)


def batch_norm_act(x: torch.Tensor, bn, training: bool, act: str = "relu6", backend: str = "auto",
                   momentum: float = 0.01, eps: float = 1e-3) -> torch.Tensor:
    """HIP BatchNorm + activation on NHWC ``x`` on the GPU, the torch expression on the CPU.

    ``backend="torch"`` forces the torch expression; ``backend="native"`` raises where the kernels do not serve."""
    if backend not in ("auto", "native", "torch"):
        raise ValueError("batch_norm_act: backend 'auto', 'native' or 'torch' expected, got {!r}".format(backend))
    if act not in ("none", "relu", "relu6"):
        raise ValueError("batch_norm_act: act 'none', 'relu' or 'relu6' expected, got {!r}".format(act))
    if backend != "torch":
        from . import native
        if x.is_cuda and native.available():
            gamma, beta, rmean, rvar, mom, ep = _bn_tensors(bn, momentum, eps)
            try:
                # NotServed is raised before a kernel runs: the running statistics are still untouched
                out = native.BatchNormActFn.apply(x, gamma, beta, rmean, rvar, bool(training), float(mom), float(ep), act)
                return out[0] if training else out
            except native.NotServed:
                if backend == "native":
                    raise
                key = (int(x.shape[-1]), bool(training), x.dtype)
                if key not in _FALLBACK_WARNED:
                    # once per form: a production layer on F.batch_norm + activation should be noticed
                    _FALLBACK_WARNED.add(key)
                    warnings.warn("batch_norm.hip does not serve C = {}, training {}, {}: the batch norm runs as the "
                                  "torch expression".format(*key))
        elif backend == "native":
            raise RuntimeError("batch_norm_act: backend 'native' needs a GPU tensor and the HIP kernel library")
    return batch_norm_act_torch(x, bn, training, act, momentum, eps)
