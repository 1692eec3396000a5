"""GroupNorm + ReLU of the head towers (``--head-norm gn``).

Statistics are per (image, pyramid level, group) over the level's pixels and the group's channels -- exactly
``F.group_norm`` on the level's own ``[B, C, h, w]`` tensor; gamma and beta are shared by the levels like the conv
weights.  :func:`group_norm_relu_packed` is the torch expression on the packed ``[B, P, C]`` pyramid: the CPU path,
the fallback for what ``csrc/kernels/group_norm.hip`` does not serve and, in float64, the oracle of its tests.
:func:`group_norm_relu` dispatches to the fused kernels (``native.GroupNormReluPackedFn``) on the GPU.
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
