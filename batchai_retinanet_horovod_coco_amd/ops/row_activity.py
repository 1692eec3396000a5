"""Row activity of the regression tower's backward (``csrc/kernels/row_activity.hip``).

The regression loss has a gradient on positive anchors only, so the gradient entering the regression final is zero
on all but a fraction of a percent of the packed pyramid rows, and each 3x3 data gradient below it widens the
support by one pixel.  A :class:`GradChain` is shared by the layers of one regression submodel forward: the final's
backward builds the row mask ``M0`` from the padded gradient it reads and, in the same two launches, its 1 .. depth
fold dilations and the active halo-tile list of every mask; layer ``k`` below the final then

* skips the 64-row K-tiles of its weight gradient whose rows of ``M_k`` are all clear (``conv_wgrad_p8.hip`` SP), and
* runs its data gradient over the halo tiles that meet ``M_k`` only (``conv_hx32.hip`` ACT), zeros elsewhere.

Both are bit-identical to the dense launches.  ``MXR_SPARSE_REG_GRAD=0`` turns it off (read per forward).

The launchers take the activity as an optional argument; inside :func:`using` it also reaches the launches that
the tuner's candidate closures make (the same winners run: no new candidate, no new key).
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import halo as _hx
from .native import ConvGeom, _chk, _p, _s, lib

MAX_DEPTH = 8      # mxr_rows_dilate's window
LAUNCHES = {"dgrad": 0, "wgrad": 0}     # launches that took an activity (tests / stats)


def enabled() -> bool:
    return os.environ.get("MXR_SPARSE_REG_GRAD", "1") == "1"


class Activity:
    """One layer's view: ``words`` (int64, one bit per packed row; word t = K-tile t), ``order`` (int32 permutation
    of the halo tiles, the ``count[0]`` active ones first), over ``M`` rows / ``ntiles`` tiles."""
    __slots__ = ("words", "order", "count", "M", "ntiles")

    def __init__(self, words, order, count, M, ntiles):
        self.words, self.order, self.count, self.M, self.ntiles = words, order, count, int(M), int(ntiles)


_CUR = [None]


class using:
    """Launches inside the block default to ``act`` (None: dense)."""
    __slots__ = ("act", "prev")

    def __init__(self, act: Optional[Activity]):
        self.act, self.prev = act, None

    def __enter__(self):
        self.prev, _CUR[0] = _CUR[0], self.act
        return self.act

    def __exit__(self, *exc):
        _CUR[0] = self.prev
        return False


def current() -> Optional[Activity]:
    return _CUR[0]


def rows_nonzero(dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 words, bit ``m % 64`` of word ``m // 64`` set where row ``m`` of the bf16 ``dy`` (rows x ld, ld % 8 == 0)
    has an element that is not +-0."""
    ld = int(dy.shape[-1])
    rows = dy.numel() // ld
    if not (dy.is_cuda and dy.dtype == torch.bfloat16 and dy.is_contiguous() and ld % 8 == 0):
        raise RuntimeError("rows_nonzero: a contiguous bf16 tensor with ld % 8 == 0")
    if out is None:
        out = torch.empty((rows + 63) // 64, dtype=torch.int64, device=dy.device)
    _chk(lib().mxr_rows_nonzero(_p(dy), rows, ld, _p(out), _s()), "rows_nonzero")
    return out


def rows_dilate(words: torch.Tensor, g: ConvGeom, nd: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[nd, nw] int64: the 1 .. nd fold 3x3 dilations of a row mask per image and level of ``g``."""
    nw = (int(g.M) + 63) // 64
    if out is None:
        out = torch.empty((nd, nw), dtype=torch.int64, device=words.device)
    if not (words.numel() >= nw and out.is_contiguous() and tuple(out.shape) == (nd, nw)):
        raise RuntimeError("rows_dilate: mask sizes do not match the geometry")
    _chk(lib().mxr_rows_dilate(_p(words), _p(out), nd, nw, ctypes.byref(g), _s()), "rows_dilate")
    return out


def halo_active_tiles(tiles: torch.Tensor, ntiles: int, masks: torch.Tensor,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """For each row mask of ``masks`` [k, nw]: (order [k, ntiles] int32 with the active tiles first, count [k] int32)."""
    k = int(masks.shape[0])
    if out is None:
        out = (torch.empty((k, ntiles), dtype=torch.int32, device=masks.device),
               torch.empty(k, dtype=torch.int32, device=masks.device))
    _chk(lib().mxr_halo_active_tiles(_p(tiles), ntiles, _p(masks), int(masks.shape[1]), k, _p(out[0]), _p(out[1]),
                                     _s()), "halo_active_tiles")
    return out


_WS: Dict[tuple, tuple] = {}


def _workspace(device, N: int, shapes, depth: int, nw: int, ntiles: int):
    """Persistent per-geometry buffers: never returned to the allocator, so the side-stream weight gradients may read
    them without stream bookkeeping (the optimizer's join orders a step's reads before the next step's writes)."""
    key = (str(device), int(N), tuple(shapes), int(depth))
    ws = _WS.get(key)
    if ws is None:
        ws = (torch.zeros((depth + 1, nw), dtype=torch.int64, device=device),
              torch.zeros((depth + 1, ntiles), dtype=torch.int32, device=device),
              torch.zeros(depth + 1, dtype=torch.int32, device=device))
        _WS[key] = ws
    return ws


class GradChain:
    """The activity of one regression-submodel backward: ``start`` at the final (level 0), ``level(k)`` for the layer
    ``k`` layers below it."""

    def __init__(self, depth: int):
        self.depth = int(depth)
        self.acts = None

    def start(self, dy: torch.Tensor, N: int, shapes: Sequence[Tuple[int, int]]) -> None:
        from .conv_launch import geom_pyramid
        self.acts = None
        ld = int(dy.shape[-1])
        if not (dy.is_cuda and dy.dtype == torch.bfloat16 and dy.is_contiguous() and ld % 8 == 0
                and 0 <= self.depth <= MAX_DEPTH):
            return
        shapes = tuple((int(h), int(w)) for h, w in shapes)
        g = geom_pyramid(N, shapes, 32, 32)
        if dy.numel() != int(g.M) * ld:
            return
        nw = (int(g.M) + 63) // 64
        tiles, nt = _hx.device_tiles(N, shapes, dy.device)
        masks, order, count = _workspace(dy.device, N, shapes, self.depth, nw, nt)
        rows_nonzero(dy, out=masks[0])
        if self.depth:
            rows_dilate(masks[0], g, self.depth, out=masks[1:])
        halo_active_tiles(tiles, nt, masks, out=(order, count))
        self.acts = [Activity(masks[k], order[k], count[k:k + 1], g.M, nt) for k in range(self.depth + 1)]

    def level(self, k: int) -> Optional[Activity]:
        if self.acts is None or not 0 <= k <= self.depth:
            return None
        return self.acts[k]
