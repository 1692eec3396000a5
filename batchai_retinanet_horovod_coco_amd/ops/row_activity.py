"""Row activity of the regression tower's backward and forward (``csrc/kernels/row_activity.hip``).

The regression loss has a gradient on positive anchors only, so the gradient entering the regression final is zero
on all but a fraction of a percent of the packed pyramid rows, and each 3x3 data gradient below it widens the
support by one pixel.  A :class:`GradChain` is shared by the layers of one regression submodel forward: the final's
backward builds the row mask ``M0`` from the padded gradient it reads and, in the same two launches, its 1 .. depth
fold dilations and the active halo-tile list of every mask; layer ``k`` below the final then

* skips the 64-row K-tiles of its weight gradient whose rows of ``M_k`` are all clear (``conv_wgrad_p8.hip`` SP), and
* runs its data gradient over the halo tiles that meet ``M_k`` only (``conv_hx32.hip`` ACT), zeros elsewhere.

Both are bit-identical to the dense launches.  ``MXR_SPARSE_REG_GRAD=0`` turns it off (read per forward).

The FORWARD of the same tower runs sparse too (:class:`FwdChain`), on a contract instead of on the data: **the loss
reads the regression output on ``state == 1`` rows only** (``smooth_l1_kernel`` / ``iou_loss_kernel``), so the final's
output is needed on the rows ``M0`` that own a positive anchor and the layer ``k`` layers below it on the k-fold
dilation ``M_k``.  The tiles that own no needed row get zeros (output and relu bitmask) from the same launch.  Nothing
in the kernels can check that contract: the Trainer enforces it -- ``Trainer.forward_backward`` hands the model the
anchor states (``RetinaNet.positive_request``) only when the losses it is about to run read the output that way, and
without the request every forward is dense.  ``MXR_SPARSE_REG_FWD=0`` turns it off (read per forward).  The positives
are a superset of the loss gradient's non-zero rows, so the backward of that step takes the forward chain's masks and
lists instead of deriving its own (same results, three launches fewer).

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
LAUNCHES = {"dgrad": 0, "wgrad": 0}     # backward launches that took an activity (tests / stats)
FWD_LAUNCHES = {"conv": 0}              # forward launches that took a needed-tiles activity
MASK_LAUNCHES = {"fwd": 0, "bwd": 0}    # mask / tile-list kernels launched by a forward chain / by a backward


def enabled() -> bool:
    return os.environ.get("MXR_SPARSE_REG_GRAD", "1") == "1"


def fwd_enabled() -> bool:
    return os.environ.get("MXR_SPARSE_REG_FWD", "1") != "0"


class Activity:
    """One layer's view: ``words`` (int64, one bit per packed row; word t = K-tile t), ``order`` (int32 permutation
    of the halo tiles, the ``count[0]`` active ones first), over ``M`` rows / ``ntiles`` tiles.

    ``need`` tells the two meanings of a list apart.  False: the conv's INPUT is zero outside the support, so the
    tiles past the count are exactly zero (a data gradient; no bias / relu / residual).  True: only the listed tiles'
    OUTPUT is needed (a forward with its bias / relu / bitmask epilogue; the others get zeros; no residual, no
    accumulate).  ``conv_launch.launch_hx32`` runs dense when the launch does not fit the activity's meaning."""
    __slots__ = ("words", "order", "count", "M", "ntiles", "need")

    def __init__(self, words, order, count, M, ntiles, need=False):
        self.words, self.order, self.count, self.M, self.ntiles = words, order, count, int(M), int(ntiles)
        self.need = bool(need)


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


def rows_positive(state: torch.Tensor, rows: int, group: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 words (the layout of :func:`rows_nonzero`; tail bits clear): packed row ``m`` is set when one of its
    anchors ``m * group .. m * group + group - 1`` of the assigner's int8 ``state`` is positive (== 1)."""
    rows, group = int(rows), int(group)
    if not (state.is_cuda and state.dtype == torch.int8 and state.is_contiguous() and rows >= 1 and group >= 1
            and state.numel() == rows * group):
        raise RuntimeError("rows_positive: a contiguous int8 state of rows * group anchors")
    nw = (rows + 63) // 64
    if out is None:
        out = torch.empty(nw, dtype=torch.int64, device=state.device)
    if not (out.is_contiguous() and out.numel() >= nw and out.dtype == torch.int64):
        raise RuntimeError("rows_positive: the mask does not hold the rows")
    _chk(lib().mxr_rows_positive(_p(state), rows, group, _p(out), _s()), "rows_positive")
    return out


def halo_active_tiles(tiles: torch.Tensor, ntiles: int, masks: torch.Tensor,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                      which: Optional[Sequence[int]] = None, ext: Optional[Sequence[int]] = None):
    """For each row mask of ``masks`` [k, nw]: (order [k, ntiles] int32 with the active tiles first, count [k] int32).

    ``which`` / ``ext`` (both or neither, at most 16 entries): list ``i`` comes from mask ``which[i]`` with the tile
    boxes extended by ``ext[i]`` pixels -- 1 (the default of every list): the tiles whose HALO meets the mask, 0: the
    tiles whose own output pixels do.  One launch either way."""
    k = int(masks.shape[0])
    if (which is None) != (ext is None):
        raise RuntimeError("halo_active_tiles: which and ext go together")
    nl = k if which is None else len(which)
    if which is not None and not (len(ext) == nl and 1 <= nl <= 16 and all(0 <= int(w) < k for w in which)
                                  and all(int(e) in (0, 1) for e in ext)):
        raise RuntimeError("halo_active_tiles: which / ext do not match the masks")
    if out is None:
        out = (torch.empty((nl, ntiles), dtype=torch.int32, device=masks.device),
               torch.empty(nl, dtype=torch.int32, device=masks.device))
    if not (out[0].is_contiguous() and out[0].numel() >= nl * ntiles and out[1].numel() >= nl):
        raise RuntimeError("halo_active_tiles: the lists do not hold the tiles")
    if which is None:
        _chk(lib().mxr_halo_active_tiles(_p(tiles), ntiles, _p(masks), int(masks.shape[1]), k, _p(out[0]), _p(out[1]),
                                         _s()), "halo_active_tiles")
    else:
        wa = (ctypes.c_int * nl)(*[int(w) for w in which])
        ea = (ctypes.c_int * nl)(*[int(e) for e in ext])
        _chk(lib().mxr_halo_active_tiles_ext(_p(tiles), ntiles, _p(masks), int(masks.shape[1]), k, nl,
                                             ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(ea, ctypes.c_void_p),
                                             _p(out[0]), _p(out[1]), _s()), "halo_active_tiles_ext")
    return out


_WS: Dict[tuple, tuple] = {}


_GEN: Dict[tuple, int] = {}      # forward workspaces: how many chains have been started into each


def _workspace(device, N: int, shapes, depth: int, nw: int, ntiles: int, fwd: bool = False):
    """Persistent per-geometry buffers: never returned to the allocator, so the side-stream weight gradients may read
    them without stream bookkeeping (the optimizer's join orders a step's reads before the next step's writes).

    A backward's data-derived chain writes its workspace in the backward; a forward chain (``fwd``: a workspace of its
    own, with one more list) writes it at the start of the NEXT step's forward.  Both are after that join: the eager
    step runs ``forward_backward`` and then ``optimizer.step()``, whose first act is ``SIDE.join()``
    (``parallel/distributed_optimizer.py``), and the next step's forward is queued on the same compute stream behind it;
    ``Trainer.graph_step`` captures the whole ``train_on_batch`` -- the join's event wait included -- so a replay ends
    joined and the next replay's mask kernels follow it on the capture stream."""
    key = (str(device), int(N), tuple(shapes), int(depth), bool(fwd))
    ws = _WS.get(key)
    if ws is None:
        nl = depth + 2 if fwd else depth + 1
        ws = (torch.zeros((depth + 1, nw), dtype=torch.int64, device=device),
              torch.zeros((nl, ntiles), dtype=torch.int32, device=device),
              torch.zeros(nl, dtype=torch.int32, device=device))
        _WS[key] = ws
    return ws + (key,) if fwd else ws


class FwdChain:
    """The needed rows of one regression-submodel forward, from the assigner's anchor states: ``start`` before the
    tower, ``need(k)`` for the layer ``k`` layers below the final (``k = 0``: the final).

    A tile is active for the forward when its UN-extended boxes meet ``M_k``.  For ``k >= 1`` that is the list of
    ``M_{k-1}`` over boxes extended by one pixel, which the backward walks anyway; the final adds one list, ``M0``
    over un-extended boxes.  ``grad(k)``: the backward's activity of the same step (``M_k``, extended boxes) while
    this chain is still the last one started into its workspace (``current``)."""

    def __init__(self, depth: int):
        self.depth = int(depth)
        self.acts = None        # need(0 .. depth)
        self.gacts = None       # grad(0 .. depth)
        self.geom = None
        self._key = self._gen = None

    def start(self, state: torch.Tensor, group: int, N: int, shapes: Sequence[Tuple[int, int]]) -> None:
        from .conv_launch import geom_pyramid
        self.acts = self.gacts = None
        shapes = tuple((int(h), int(w)) for h, w in shapes)
        g = geom_pyramid(N, shapes, 32, 32)
        M, d = int(g.M), self.depth
        if not (state is not None and state.is_cuda and state.dtype == torch.int8 and state.is_contiguous()
                and int(group) >= 1 and state.numel() == M * int(group) and 0 <= d <= MAX_DEPTH):
            return
        nw = (M + 63) // 64
        tiles, nt = _hx.device_tiles(N, shapes, state.device)
        masks, order, count, key = _workspace(state.device, N, shapes, d, nw, nt, fwd=True)
        rows_positive(state, M, group, out=masks[0])
        if d:
            rows_dilate(masks[0], g, d, out=masks[1:])
        # lists 0 .. d: M_k over extended boxes; list d + 1: M0 over un-extended boxes
        halo_active_tiles(tiles, nt, masks, out=(order, count), which=list(range(d + 1)) + [0], ext=[1] * (d + 1) + [0])
        MASK_LAUNCHES["fwd"] += 3 if d else 2
        self._key = key
        self._gen = _GEN[key] = _GEN.get(key, 0) + 1
        self.geom = (int(N), shapes)
        lst = [d + 1] + list(range(d))      # need(k)'s list
        self.acts = [Activity(masks[k], order[lst[k]], count[lst[k]:lst[k] + 1], M, nt, need=True)
                     for k in range(d + 1)]
        self.gacts = [Activity(masks[k], order[k], count[k:k + 1], M, nt) for k in range(d + 1)]

    def current(self) -> bool:
        return self.acts is not None and _GEN.get(self._key) == self._gen

    def need(self, k: int) -> Optional[Activity]:
        if self.acts is None or not 0 <= k <= self.depth:
            return None
        return self.acts[k]


class GradChain:
    """The activity of one regression-submodel backward: ``start`` at the final (level 0), ``level(k)`` for the layer
    ``k`` layers below it."""

    def __init__(self, depth: int, fwd: Optional[FwdChain] = None):
        self.depth = int(depth)
        self.acts = None
        # the forward chain of the same step: its positives are a superset of the gradient's non-zero rows
        self.fwd = fwd

    def start(self, dy: torch.Tensor, N: int, shapes: Sequence[Tuple[int, int]]) -> None:
        from .conv_launch import geom_pyramid
        self.acts = None
        f = self.fwd
        if (f is not None and f.depth == self.depth and f.current()
                and f.geom == (int(N), tuple((int(h), int(w)) for h, w in shapes))):
            self.acts = f.gacts      # no mask kernels: the forward's masks and lists
            return
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
        MASK_LAUNCHES["bwd"] += 3 if self.depth else 2
        self.acts = [Activity(masks[k], order[k], count[k:k + 1], g.M, nt) for k in range(self.depth + 1)]

    def level(self, k: int) -> Optional[Activity]:
        if self.acts is None or not 0 <= k <= self.depth:
            return None
        return self.acts[k]
