"""Weight and bias gradients of the convolutions: split-K implicit GEMMs with slab
reductions, the halo-staged 3x3 form, the 64-channel 3x3 kernel, column-sum bias gradients, and their
delivery into the flat gradient buffer (gradient sinks, side stream) -- split out of ``native_conv``.

One builder, :func:`wgrad_candidates`, offers every weight-gradient form of a geometry (:data:`_KINDS`, the library
form, the caller's extras) as fresh-tensor or accumulate-into-slot candidates, whole or one name at a time.  One
function, :func:`_deliver`, runs a launch into gradient slots and notifies the parameters, on the side stream or the
current one; the entries (:func:`deliver_wgrad`, :func:`deliver_wgrad_bias_fused`, :func:`run_wgrad_proj`,
:func:`deliver_bias_grad`, ``fp8.deliver_pyramid_wgrad``) only say which slots, which reads, which stream and what
to launch.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import native as _n
from .native import ConvGeom, _chk, _p, _s, lib, zero_page, c_int, c_ll, c_vp
from .side_stream import SIDE, _NULL
from . import row_activity as _ra
from .conv_launch import (_bind, _miopen_wgrad, _only, geom_single)


_WGRAD_TILE = {0: (128, 128), 1: (128, 64), 2: (64, 128)}   # variant -> (BK, BCO)

def _splits(g: ConvGeom, bk: int, bco: int) -> int:
    K = g.kh * g.kw * g.cin
    tiles = ((K + bk - 1) // bk) * ((g.cout + bco - 1) // bco)
    steps = (g.M + 63) // 64
    target = 1024
    s = max(1, -(-target // tiles))
    return int(max(1, min(s, steps // 4 if steps >= 4 else 1, 256)))


# variant -> (TK, TC) of conv_wgrad_pipe.hip (5 / 6: DMA interleaved between MFMA groups, 7: interleaved +
# s_setprio, 8 / 9: s_setprio around the MFMA block, 10-12: narrow 4-wave tiles for 64-channel layers,
# 13-15: two blocks per CU -- 128 x 128, and 256 x 128 / 128 x 256 on 3-deep rings)

_WGRAD_PIPE_TILE = {3: (256, 256), 4: (256, 128), 5: (256, 256), 6: (256, 128), 7: (256, 256), 8: (256, 256),
                    9: (256, 128), 10: (256, 64), 11: (128, 64), 12: (64, 64), 13: (128, 128), 14: (256, 128),
                    15: (128, 256)}
# phase-pipelined 256 k x 256 co wgrad (conv_wgrad_p8.hip): variant -> kernel variant (1 = s_setprio)

_WGRAD_P8 = {20: 0, 21: 1, 22: 2, 23: 3, 24: 4, 25: 5}
# resident blocks per CU the split count aims for (narrow / small-ring tiles run several per CU)

_WGRAD_PIPE_OCC = {10: 2, 11: 3, 12: 4, 13: 2, 14: 2, 15: 2}

# slab-free ("direct") forms of conv_wgrad_pipe.hip: variant -> ((TK, TC), kernel variant, the slab variant of the
# same tile).  One split over the whole pixel range, the epilogue writes / accumulates the gradient itself: no
# workspace, no reduce launch.
_WGRAD_DIRECT = {30: ((128, 128), 0, 13), 31: ((64, 64), 1, 12)}
# candidates only where the tile count alone gives a useful grid and the pixel range one block walks is short.
# Sweep (profiles/r7_wgrad_direct_sweep.txt, R50-FPN layers at 1 / 2 / 4 images): the direct form wins up to 1,092
# pixels (1.05-1.56x at >= 144 tiles) and loses from 2,100 pixels on (<= 0.82x) and at 128 tiles / 1,050 pixels
# (0.70x).  The bounds only prune hopeless races; the tuner decides.
DIRECT_MIN_TILES = 128       # 64 x 64 tiles of the output
DIRECT_MAX_PIXELS = 1536


def direct_covers(g: ConvGeom) -> bool:
    """Single-geometry keys the slab-free weight gradient is raced for (the small-M layers of a one- to four-image
    step: stage 4 / 5, FPN P5-P7)."""
    if g.nlev != 1 or g.cin % 8 or g.ostride != 1:
        return False
    K = g.kh * g.kw * g.cin
    tiles = -(-K // 64) * -(-g.cout // 64)
    return tiles >= DIRECT_MIN_TILES and g.M <= DIRECT_MAX_PIXELS


def _wgrad_variants(g: ConvGeom):
    vs = list(_WGRAD_TILE) + list(_WGRAD_PIPE_TILE) + list(_WGRAD_P8)
    return vs + list(_WGRAD_DIRECT) if direct_covers(g) else vs


def _splits_pipe(g: ConvGeom, tk: int, tc: int, occ: int = 1) -> int:
    """Pixel splits so the grid is ~192 x ``occ`` blocks (``occ`` blocks on three quarters of the 256 CUs),
    each split >= 8 sub-stages of 32 rows.  The weight gradients run on the side stream next to the data-gradient chain:
    a grid that leaves a quarter of the CUs to the concurrent dgrad kernels also halves the split-K slab
    traffic of a full-chip grid's extra splits (bench sweep: 128 / 160 / 192 / 224 / 256 / 384 blocks ->
    434 / 446 / 457-458 / 446 / 452 / 433 img/s)."""
    K = g.kh * g.kw * g.cin
    tiles = ((K + tk - 1) // tk) * ((g.cout + tc - 1) // tc)
    nsub = (g.M + 31) // 32
    target = int(os.environ.get("MXR_WGRAD_PIPE_BLOCKS", "192")) * occ
    if g.nlev > 1:       # the packed head layers (a separate target only for the sweep, scripts/gpu_sweep_wgrad_blocks.sh)
        target = int(os.environ.get("MXR_WGRAD_HEAD_BLOCKS", str(target)))
    s = max(1, round(target / tiles))
    return int(max(1, min(s, nsub // 8 if nsub >= 8 else 1, 512 * occ)))

def conv_wgrad(x, dy, g: ConvGeom, scale: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
               accumulate: bool = False, variant: Optional[int] = None, bias_out: Optional[torch.Tensor] = None,
               bias_accumulate: bool = False, splits: Optional[int] = None, rowmask=None) -> torch.Tensor:
    """fp32 dW (OHWI) = scale[co] * sum_m dY (x) im2col(X); dY may have cout % 8 != 0 (padded).
    ``splits``: the pixel-split count of the split-K forms (default: the per-kernel heuristic).
    ``bias_out`` (phase-pipelined variants, see :data:`_WGRAD_P8`, cout % 4 == 0): the unscaled bias
    gradient sum_m dY[m, :cout] is computed by the same kernel from the dY tiles it stages anyway.
    ``rowmask`` (an ``ops.row_activity.Activity``; default: the one of the enclosing ``row_activity.using`` block):
    the rows of ``dy`` outside it are all zero -- the phase-pipelined variants skip the 64-row K-tiles without a set
    row (bit-identical to the dense walk); the other variants run dense."""
    cout = g.cout
    K = g.kh * g.kw * g.cin
    ldy = dy.shape[-1]
    if ldy % 8:
        dy = F.pad(dy, (0, 8 - ldy % 8))
        ldy = dy.shape[-1]
    dy = dy.contiguous()
    if variant is None:
        variant = 1 if cout <= 64 else (2 if K <= 64 else 0)
    if out is None:
        out = torch.empty((cout, g.kh, g.kw, g.cin), dtype=torch.float32, device=dy.device)
    sc = None if scale is None else scale.float().contiguous()
    if bias_out is not None and (variant not in _WGRAD_P8 or cout % 4 or bias_out.numel() != cout
                                 or bias_out.dtype != torch.float32 or not bias_out.is_contiguous()):
        raise RuntimeError("conv_wgrad: the fused bias gradient needs a phase-pipelined variant, cout % 4 == 0 "
                           "and a contiguous fp32 (cout,) output")
    if splits is not None and (splits < 1 or splits > max(1, (g.M + 31) // 32)):
        raise RuntimeError("conv_wgrad: splits must be between 1 and the number of 32-pixel sub-stages")
    if variant in _WGRAD_DIRECT:
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != cout * K:
            raise RuntimeError("conv_wgrad: the direct form writes a contiguous fp32 (cout, K) gradient")
        _chk(lib().mxr_conv_wgrad_pipe_direct(_p(x), _p(dy), ldy, _p(out), _p(sc), int(accumulate),
                                              _p(zero_page(dy.device)), ctypes.byref(g), _WGRAD_DIRECT[variant][1],
                                              _s()), "conv_wgrad_pipe_direct")
        return out
    if variant in _WGRAD_P8:
        splits = splits or _splits_pipe(g, 256, 256)
        nb = 0 if bias_out is None else splits * cout
        part = torch.empty(splits * cout * K + nb, dtype=torch.float32, device=dy.device)
        act = rowmask if rowmask is not None else _ra.current()
        if act is not None and act.M == int(g.M) and dy.numel() == int(g.M) * ldy:
            _ra.LAUNCHES["wgrad"] += 1
            _chk(lib().mxr_conv_wgrad_p8_bias_act(_p(x), _p(dy), ldy, _p(part), splits, _p(out), _p(sc),
                                                  int(accumulate), _p(zero_page(dy.device)), ctypes.byref(g),
                                                  _WGRAD_P8[variant], _p(bias_out), int(bias_accumulate),
                                                  _p(act.words), _s()), "conv_wgrad_p8_act")
            return out
        _chk(lib().mxr_conv_wgrad_p8_bias(_p(x), _p(dy), ldy, _p(part), splits, _p(out), _p(sc), int(accumulate),
                                          _p(zero_page(dy.device)), ctypes.byref(g), _WGRAD_P8[variant],
                                          _p(bias_out), int(bias_accumulate), _s()),
             "conv_wgrad_p8")
        return out
    if variant in _WGRAD_PIPE_TILE:
        tk, tc = _WGRAD_PIPE_TILE[variant]
        splits = splits or _splits_pipe(g, tk, tc, _WGRAD_PIPE_OCC.get(variant, 1))
        part = torch.empty(splits * cout * K, dtype=torch.float32, device=dy.device)
        _chk(lib().mxr_conv_wgrad_pipe(_p(x), _p(dy), ldy, _p(part), splits, _p(out), _p(sc), int(accumulate),
                                       _p(zero_page(dy.device)), ctypes.byref(g), variant - 3, _s()),
             "conv_wgrad_pipe")
        return out
    bk, bco = _WGRAD_TILE[variant]
    splits = splits or _splits(g, bk, bco)
    part = torch.empty(splits * cout * K, dtype=torch.float32, device=dy.device)
    _chk(_bind().mxr_conv_wgrad(_p(x), _p(dy), ldy, _p(part), splits, _p(out), _p(sc), int(accumulate),
                                _p(zero_page(dy.device)), ctypes.byref(g), variant, _s()), "conv_wgrad")
    return out

def _hip_names(g: ConvGeom, only):
    if only is None:
        return ["hip%d" % v for v in _wgrad_variants(g)]
    return [only] if only[:3] == "hip" and only[3:].isdigit() and int(only[3:]) in _wgrad_variants(g) else []

def _one_name(name: str, covers):
    return lambda g, only: [name] if (only is None or only == name) and covers(g) else []

# The native kinds of weight-gradient candidate, in race order.  Per kind: the names offered for a geometry (all of
# them, or just ``only``), the launcher of a name into ``out`` (None: a fresh tensor), and the shape the kernel takes
# the parameter's gradient slot in (None: as it is).  Launchers are looked up when they run (tests replace them).
_KINDS = (
    (_hip_names,
     lambda n, x, dy, g, scale, out, acc: conv_wgrad(x, dy, g, scale, out=out, accumulate=acc, variant=int(n[3:])),
     None),
    (_one_name("w64", lambda g: w64_covers(g)),
     lambda n, x, dy, g, scale, out, acc: wgrad3x3_c64(x, dy, scale, out=out, accumulate=acc),
     lambda g: (64, 3, 3, 64)),
    (_one_name("whalo", lambda g: whalo_covers(g)),
     lambda n, x, dy, g, scale, out, acc: halo_wgrad(x, dy, g, scale, out=out, accumulate=acc),
     lambda g: (g.cout, 3, 3, g.cin)),
)
_LIB = "miopen"
_ORDER = {False: _KINDS + (_LIB,), True: _KINDS[:1] + (_LIB,) + _KINDS[1:]}      # by "accumulating"

def wgrad_candidates(x, dy, g, scale, only: Optional[str] = None, sink: Optional[torch.Tensor] = None, lib_fn=None,
                     extra=None):
    """{name: launch} of the weight gradient of ``g``, in race order: the native kinds (:data:`_KINDS`), the library
    form ``miopen`` when ``lib_fn`` is given, then the caller's ``extra`` ``{name: fn}``.  Without ``sink`` every
    candidate returns a fresh fp32 gradient; with it every candidate accumulates into ``sink`` (a parameter's slot,
    or a scratch copy of it) -- the native kinds through their kernels' accumulate form, ``lib_fn`` and ``extra``
    (which return a fresh tensor) by adding their result.  ``only``: build that one candidate and nothing else
    ({} when it is not offered here); the tuned dispatch's fast path (``conv_launch._only``).
    The two forms differ in where ``miopen`` sits (after the native kinds / right after the ``hipN`` names): the
    recorded race orders (tests/fixtures/wgrad_candidates.json), which decide ties and untuned captures."""
    acc = sink is not None
    c = {}

    def fresh(name, fn):
        if fn is not None and (only is None or only == name):
            c[name] = (lambda: sink.add_(fn())) if acc else fn
    for kind in _ORDER[acc]:
        if kind is _LIB:
            fresh(_LIB, lib_fn)
            continue
        names, launch, view = kind
        for name in names(g, only):
            out = sink.view(view(g)) if acc and view is not None else sink
            c[name] = lambda name=name, launch=launch, out=out: launch(name, x, dy, g, scale, out, acc)
    for name, fn in (extra or {}).items():
        fresh(name, fn)
    return c

def whalo_covers(g: ConvGeom) -> bool:
    """3x3 / stride 1 / pad 1 with Cin % 64 == 0 and Cout >= 64 (single level or packed pyramid):
    csrc/kernels/wgrad_halo.hip."""
    return (g.kh == 3 and g.kw == 3 and g.stride == 1 and g.pt == 1 and g.pl == 1 and g.ostride == 1
            and g.cin % 64 == 0 and g.cout >= 64
            and all(g.H[l] == g.Ho[l] and g.W[l] == g.Wo[l] for l in range(g.nlev)))

_WH_TILES = {}

def _wh_box(h: int, w: int):
    """R x C box for a level: 2 x 64 where the level is at least 64 wide, else full-width boxes of as
    many rows as fit 128 slots / 264 halo rows.  (Measured: boxes narrower than 64 columns that waste
    fewer slots are still slower -- the per-step slot -> row / col division and shorter halo rows.)"""
    if w >= 64:
        return 2, 64
    r = max(1, min(128 // w, h))
    while r > 1 and (r + 2) * (w + 2) > 264:
        r -= 1
    return r, w

def halo_wgrad_tiles(N: int, shapes, device):
    """(tile table int4 {image, level, oy0, ox0}, per-level (R, C) boxes, #leading 2 x 64 tiles): the
    tiles of levels >= 64 wide first (the kernel's compile-time box), then the narrow levels; image /
    level / row order within each so consecutive tiles share halo rows."""
    key = (N, tuple(shapes), str(device))
    t = _WH_TILES.get(key)
    if t is None:
        boxes = [_wh_box(h, w) for h, w in shapes]
        def rows(wide):
            return [(b, l, y, x) for b in range(N) for l, (h, w) in enumerate(shapes) if (boxes[l][1] == 64) == wide
                    for y in range(0, h, boxes[l][0]) for x in range(0, w, boxes[l][1])]
        wide = rows(True)
        t = (torch.tensor(wide + rows(False), dtype=torch.int32, device=device), boxes, len(wide))
        _WH_TILES[key] = t
    return t

def halo_wgrad(x, dy, g: ConvGeom, scale=None, out: Optional[torch.Tensor] = None, accumulate: bool = False,
               splits: Optional[int] = None) -> torch.Tensor:
    """fp32 (cout, 3, 3, cin) weight gradient from halo-staged tiles (``dy`` may be wider than cout)."""
    if not whalo_covers(g):
        raise RuntimeError("wgrad_halo: geometry not covered")
    shapes = [(g.H[l], g.W[l]) for l in range(g.nlev)]
    N = int(g.M) // g.out_img
    ldy = dy.shape[-1]
    if ldy % 8:
        dy = F.pad(dy, (0, 8 - ldy % 8))
        ldy = dy.shape[-1]
    x, dy = x.contiguous(), dy.contiguous()
    if not (x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16 and x.numel() == N * g.in_img * g.cin
            and dy.numel() == N * g.out_img * ldy and g.in_img == g.out_img):
        raise RuntimeError("wgrad_halo: operands do not match the geometry")
    tiles, boxes, nwide = halo_wgrad_tiles(N, shapes, x.device)
    n_co, n_ci = -(-g.cout // 128), g.cin // 64
    if splits is None:
        splits = max(1, min(int(tiles.shape[0]), round(256 / (n_co * n_ci))))
    splits = max(splits, int(nwide > 0) + int(nwide < int(tiles.shape[0])))
    ws = torch.empty(splits * g.cout * 9 * g.cin, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty((g.cout, 3, 3, g.cin), dtype=torch.float32, device=x.device)
        accumulate = False
    sc = None if scale is None else scale.float().contiguous()
    Hs = (ctypes.c_int * 5)(*[g.H[l] for l in range(5)])
    Ws = (ctypes.c_int * 5)(*[g.W[l] for l in range(5)])
    Os = (ctypes.c_int * 5)(*[g.in_off[l] for l in range(5)])
    Rs = (ctypes.c_int * 5)(*([b[0] for b in boxes] + [1] * (5 - len(boxes))))
    Cs = (ctypes.c_int * 5)(*([b[1] for b in boxes] + [1] * (5 - len(boxes))))
    _chk(lib().mxr_wgrad_halo(_p(x), _p(dy), ldy, _p(tiles), int(tiles.shape[0]), nwide, splits, g.nlev, Hs, Ws, Os, Rs, Cs,
                              g.in_img, g.cin, g.cout, _p(ws), _p(sc), _p(out), int(accumulate), _s()), "wgrad_halo")
    return out

def w64_covers(g: ConvGeom) -> bool:
    """3x3 / stride 1 / pad 1, 64 -> 64 channels, one level: csrc/kernels/wgrad_narrow.hip."""
    return (g.nlev == 1 and g.kh == 3 and g.kw == 3 and g.stride == 1 and g.pt == 1 and g.pl == 1 and g.cin == 64
            and g.cout == 64 and g.H[0] == g.Ho[0] and g.W[0] == g.Wo[0] and g.ostride == 1)

def wgrad3x3_c64(x, dy, scale=None, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """fp32 (64, 3, 3, 64) weight gradient of a 64-channel 3x3/s1 conv, ``scale`` (frozen BN) folded in."""
    N, H, W, C = x.shape
    if not (C == 64 and tuple(dy.shape) == (N, H, W, 64) and x.is_contiguous() and dy.is_contiguous()
            and x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16):
        raise RuntimeError("wgrad3x3_c64: operands not covered")
    ntiles = N * ((H + 1) // 2) * ((W + 63) // 64)
    ws = torch.empty(min(ntiles, 256) * 64 * 576, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty((64, 3, 3, 64), dtype=torch.float32, device=x.device)
        accumulate = False
    sc = None if scale is None else scale.float().contiguous()
    _chk(lib().mxr_wgrad3x3_c64(_p(x), _p(dy), _p(ws), _p(sc), _p(out), N, H, W, int(accumulate), _s()),
         "wgrad3x3_c64")
    return out

def bias_grad(dy: torch.Tensor, scale: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              accumulate: bool = False, channels: Optional[int] = None) -> torch.Tensor:
    """``channels``: the first ``channels`` of each (wider, zero-padded) row of ``dy``."""
    ld = dy.shape[-1]
    C = channels or ld
    M = dy.numel() // ld
    C8 = (C + 7) // 8 * 8          # padded rows: sum the zero columns up to the next 8 too, write C
    if C8 > ld or C8 // 8 > 256 or ld % 8:
        db = dy.float().reshape(M, ld)[:, :C].sum(0)
        db = db * scale if scale is not None else db
        if out is None:
            return db
        return out.add_(db) if accumulate else out.copy_(db)
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=dy.device)
    part = torch.empty(512 * C8, dtype=torch.float32, device=dy.device)
    sc = None if scale is None else scale.float().contiguous()
    _chk(_bind().mxr_bias_grad(_p(dy.contiguous()), M, C8, ld, C, _p(part), _p(out), _p(sc), int(accumulate), _s()),
         "bias_grad")
    return out

def _sink(param):
    gs = _n.grad_sinks()
    return gs.get(param) if gs is not None else None

def _side(sink, param) -> bool:
    """Whether this weight gradient goes to the side stream: not for parameters tagged ``mxr_main_wgrad``
    (models.resnet: the last blocks of the backward, whose weight gradients would otherwise queue at the
    end of the side stream's backlog while the compute stream idles before the optimizer)."""
    return SIDE.usable(sink) and not getattr(param, "mxr_main_wgrad", False)

def _deliver(params, side: bool, device, reads, fn) -> None:
    """The one delivery path of every gradient that accumulates into its parameter's slot: run ``fn`` (the launch
    into the slots of ``params``), then notify each parameter in order -- inside a side-stream region when ``side``
    (``ops.side_stream``: ``reads`` = the compute-stream tensors ``fn`` reads, and the notify inside the region so a
    bucket-ready event covers both streams), else on the current stream."""
    with SIDE.run(device, *reads) if side else _NULL:
        fn()
        gs = _n.grad_sinks()
        for p in params:
            gs.notify(p)

def _tuned(key, make, *slots):
    """(the accumulating candidates ``make(*slots)``, whether they were raced): a set the tuner would time is first
    raced on scratch copies of the slots; the caller then runs the winner for real -- serially, like every first
    sight of a shape."""
    from .conv_tuner import TUNER
    c = make(*slots)
    if not TUNER.needs_tuning(key, c):
        return c, False
    TUNER.run(key, make(*[s.clone() for s in slots]))
    return c, True

def deliver_bias_grad(param, dy, scale=None, channels: Optional[int] = None):
    """Bias gradient for ``param``: straight into its flat-gradient slot when a sink is active
    (returns None so autograd does not add it again), else a tensor."""
    sink = _sink(param)
    if sink is None:
        return bias_grad(dy, scale, channels=channels)
    _deliver((param,), SIDE.usable(dy), dy.device, (dy, scale),
             lambda: bias_grad(dy, scale, out=sink, accumulate=True, channels=channels))
    return None

def deliver_wgrad(key, x, dy, g: ConvGeom, scale, param, reads, lib_fn, extra=None):
    """Run the tuned wgrad of ``g`` (:func:`wgrad_candidates` with ``lib_fn`` / ``extra``); with a gradient sink for
    ``param`` accumulate into it and return None.  Once the sink form is tuned it runs on the side stream
    (``ops.side_stream``), overlapped with the data gradients; ``reads`` = the compute-stream tensors it reads."""
    from .conv_tuner import TUNER
    sink = _sink(param)
    if sink is None:
        return TUNER.run(key, wgrad_candidates(x, dy, g, scale, lib_fn=lib_fn, extra=extra))
    key = key + "|s"        # accumulate-into-sink forms: the library path pays an extra add

    def make(slot, only=None):
        return wgrad_candidates(x, dy, g, scale, only=only, sink=slot, lib_fn=lib_fn, extra=extra)
    only = _only(key)
    c, raced = (make(sink, only) if only is not None else None), False
    if not c:
        c, raced = _tuned(key, make, sink)
    _deliver((param,), not raced and _side(sink, param), sink.device, reads, lambda: TUNER.run(key, c))
    return None

def _is_p8(name: str) -> bool:
    return name.startswith("hip") and name[3:].isdigit() and int(name[3:]) in _WGRAD_P8

def deliver_wgrad_bias_fused(key, x, dy, g: ConvGeom, wparam, bparam) -> bool:
    """Weight AND bias gradient of an unscaled conv in one kernel, when the tuned sink winner for ``key``
    is a phase-pipelined variant (conv_wgrad_p8.hip BIAS: the bias sums come from the dY tiles the wgrad
    stages anyway, instead of a separate colsum pass over all of dY) and both parameters have gradient
    sinks.  Accumulates into both sinks (on the side stream when usable) and returns True; False = not
    applicable, the caller runs the separate paths.  ``MXR_WGRAD_FUSED_BIAS=0`` disables it."""
    from .conv_tuner import TUNER
    if g.cout % 4 or os.environ.get("MXR_WGRAD_FUSED_BIAS", "1") == "0":
        return False
    gs = _n.grad_sinks()
    if gs is None:
        return False
    ws, bs = gs.get(wparam), gs.get(bparam)
    if ws is None or bs is None or bs.numel() != g.cout:
        return False
    key = key + "|s"
    win = TUNER.winner(key)
    if win is not None and not _is_p8(win):
        # a near-tie race winner without the fused bias form loses the separate bias pass over all of dY:
        # adopt the fastest phase-pipelined candidate within that pass's time (ConvTuner.prefer)
        t = TUNER.timings.get(TUNER.borrowed.get(key, key), {})
        p8 = sorted((v, n) for n, v in t.items() if isinstance(v, float) and _is_p8(n))
        if p8 and TUNER.prefer(key, p8[0][1], dy.numel() * dy.element_size() / 4.0e9):
            win = p8[0][1]
    if win is None or not _is_p8(win):
        return False
    v = int(win[3:])
    TUNER.calls[key] = TUNER.calls.get(key, 0) + 1
    _deliver((wparam, bparam), _side(ws, wparam), ws.device, (x, dy),
             lambda: conv_wgrad(x, dy, g, None, out=ws, accumulate=True, variant=v, bias_out=bs, bias_accumulate=True))
    return True

def run_wgrad(x, dy, w, stride, pads, scale, param=None) -> Optional[torch.Tensor]:
    """Tuned fp32 weight gradient (OHWI), scaled by the folded frozen-BN scale.  With an active
    gradient sink for ``param`` it is accumulated into the flat gradient buffer (returns None)."""
    from .conv_tuner import TUNER
    N, H, W, cin = x.shape
    cout, kh = w.shape[0], w.shape[1]
    Ho, Wo = dy.shape[1], dy.shape[2]
    g = geom_single(N, H, W, Ho, Wo, kh, stride, pads, cin, cout)
    key = TUNER.key("wgrad", N, H, W, cin, cout, kh, stride, tuple(pads))
    return deliver_wgrad(key, x, dy, g, scale, param, (x, dy, scale),
                         lambda: _miopen_wgrad(x, w, dy, stride, pads, scale))

def run_wgrad_bias_fused(x, dy, w, stride, pads, scale, param, bias_param) -> bool:
    """:func:`deliver_wgrad_bias_fused` for a single-geometry conv (the FPN convs: biased, unscaled);
    True = both gradients delivered, False = the caller runs :func:`run_wgrad` and the bias pass."""
    if scale is not None:
        return False
    from .conv_tuner import TUNER
    N, H, W, cin = x.shape
    cout, kh = w.shape[0], w.shape[1]
    g = geom_single(N, H, W, dy.shape[1], dy.shape[2], kh, stride, pads, cin, cout)
    key = TUNER.key("wgrad", N, H, W, cin, cout, kh, stride, tuple(pads))
    return deliver_wgrad_bias_fused(key, x, dy, g, param, bias_param)


# the projection blocks' two weight gradients as ONE dual-source GEMM (a switch for same-process A/Bs)
PROJ_WGRAD = True
PROJ_WGRAD_MIN_PX = 40000
_WGRAD_DUAL = (0, 1, 2, 4)


def proj_wgrad_fusable(h2, x, dy, w2c, w1, stride) -> bool:
    """:func:`run_wgrad_proj`'s contract (1x1 convs, bf16, both channel counts multiples of 8) with gradient sinks
    for both weights (the training step)."""
    from . import conv_launch as _cl
    if not (PROJ_WGRAD and _cl.PROJ_FUSED and dy.is_cuda and dy.dtype == torch.bfloat16):
        return False
    if w2c.shape[1] != 1 or w2c.shape[2] != 1 or w1.shape[1] != 1 or w1.shape[2] != 1:
        return False
    # (res5a at B=16 -- 16,800 pixels, K = 512 + 1024 -- measured 0.150 ms fused vs 0.127 ms for the two separate
    # weight gradients: below ~40k pixels the split-K grid of the long-K fused GEMM loses, profiles/r6_conv_budget_dual.txt)
    return (h2.shape[-1] % 8 == 0 and x.shape[-1] % 8 == 0 and dy.shape[-1] % 8 == 0
            and dy.shape[0] * dy.shape[1] * dy.shape[2] >= PROJ_WGRAD_MIN_PX
            and tuple(h2.shape[:3]) == tuple(dy.shape[:3])
            and (x.shape[1] - 1) // stride + 1 == dy.shape[1] and (x.shape[2] - 1) // stride + 1 == dy.shape[2])


def run_wgrad_proj(h2, x, dy, stride, s2c, s1, p2c, p1) -> bool:
    """Both weight gradients of a projection block from ONE read of its output gradient ``dy``
    (conv_wgrad_p8.hip DS form): dW2c over the branch2b output ``h2`` and dW1 over the stride-``stride`` 1x1 im2col of
    the block input ``x`` as one split-K GEMM over the concatenated K, reduced straight into both gradient sinks
    (scaled by the two frozen-BN scales).  On the side stream like the single weight gradients.  False when a sink is
    missing (the caller runs the two separate weight gradients)."""
    from .conv_tuner import TUNER
    k1 = int(h2.shape[-1])
    gs = _n.grad_sinks()
    o1 = gs.get(p2c) if gs is not None else None
    o2 = gs.get(p1) if gs is not None else None
    if o1 is None or o2 is None:
        return False
    N, H, W, cin = x.shape
    cout = int(dy.shape[-1])
    Ho, Wo = int(dy.shape[1]), int(dy.shape[2])
    g = geom_single(N, H, W, Ho, Wo, 1, stride, (0, 0, 0, 0), cin, cout)
    K = k1 + cin
    splits = _splits_pipe(_kgeom(g, K), 256, 256)
    h2, x, dy = h2.contiguous(), x.contiguous(), dy.contiguous()
    sc1 = None if s2c is None else s2c.float().contiguous()
    sc2 = None if s1 is None else s1.float().contiguous()
    zp = _p(zero_page(dy.device))

    def cand(v, d1, d2):
        def f():
            part = torch.empty(splits * cout * K, dtype=torch.float32, device=dy.device)
            _chk(lib().mxr_conv_wgrad_p8_dual(_p(x), _p(h2), k1, _p(dy), cout, _p(part), splits, _p(d1), _p(d2),
                                              _p(sc1), _p(sc2), 1, zp, ctypes.byref(g), v, _s()), "conv_wgrad_p8_dual")
            return d1
        return f
    key = TUNER.key("wgradp", N, Ho, Wo, k1, cin, cout, stride, H, W) + "|s"
    win = TUNER.winner(key)
    if win is not None and win.startswith("p8d_") and int(win[4:]) in _WGRAD_DUAL:
        c, raced = {win: cand(int(win[4:]), o1, o2)}, False
    else:
        c, raced = _tuned(key, lambda d1, d2: {"p8d_%d" % v: cand(v, d1, d2) for v in _WGRAD_DUAL}, o1, o2)
    _deliver((p2c, p1), not raced and _side(o1, p2c), o1.device, (h2, x, dy, sc1, sc2), lambda: TUNER.run(key, c))
    return True


def _kgeom(g: ConvGeom, K: int) -> ConvGeom:
    """``g`` with its K (kh * kw * cin) replaced by ``K`` -- for the split count of a dual-source GEMM."""
    h = ConvGeom.from_buffer_copy(g)
    h.cin = K
    return h
