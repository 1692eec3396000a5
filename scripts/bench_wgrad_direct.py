#!/usr/bin/env python
"""Slab-free ("direct") weight gradient vs the split-K slab forms at the small-M layers of a 1 / 2 / 4-image
R50-FPN step at 800 x 1333 (stage 3-5, FPN P3-P7): isolated kernel time of every candidate accumulating into a
gradient slot (events around batches of launches, median of repeats).  Per layer: pixels M, 64 x 64 output tiles,
the fastest slab candidate, the direct tiles and best-slab / best-direct.  The sweep behind
``ops.conv_wgrad.direct_covers``'s two bounds (DIRECT_MIN_TILES, DIRECT_MAX_PIXELS).

usage: bench_wgrad_direct.py [--batches 1,2,4] [--reps 7] [--inner 20]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd.ops import conv_wgrad as CW  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402

# (name, H, W, cin, cout, k, stride) at one 800 x 1333 image
LAYERS = [
    ("res3 1x1 128>512", 100, 167, 128, 512, 1, 1), ("res3 3x3 128", 100, 167, 128, 128, 3, 1),
    ("res3 1x1 512>128", 100, 167, 512, 128, 1, 1),
    ("res4 1x1 256>1024", 50, 84, 256, 1024, 1, 1), ("res4 3x3 256", 50, 84, 256, 256, 3, 1),
    ("res4 1x1 1024>256", 50, 84, 1024, 256, 1, 1), ("res4a 1x1/2 512>1024", 100, 167, 512, 1024, 1, 2),
    ("res5 1x1 512>2048", 25, 42, 512, 2048, 1, 1), ("res5 3x3 512", 25, 42, 512, 512, 3, 1),
    ("res5 1x1 2048>512", 25, 42, 2048, 512, 1, 1), ("res5a 1x1/2 1024>2048", 50, 84, 1024, 2048, 1, 2),
    ("fpn C5 1x1 2048>256", 25, 42, 2048, 256, 1, 1), ("fpn C4 1x1 1024>256", 50, 84, 1024, 256, 1, 1),
    ("fpn C3 1x1 512>256", 100, 167, 512, 256, 1, 1), ("fpn P5 3x3 256", 25, 42, 256, 256, 3, 1),
    ("fpn P4 3x3 256", 50, 84, 256, 256, 3, 1), ("fpn P3 3x3 256", 100, 167, 256, 256, 3, 1),
    ("fpn P6 3x3/2 2048>256", 25, 42, 2048, 256, 3, 2), ("fpn P7 3x3/2 256", 13, 21, 256, 256, 3, 2),
]


def timeit(fn, reps, inner):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    N.load(required=True)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    print("%-24s %2s %6s %5s  %-16s %s  slab/direct" % ("layer", "B", "M", "tiles", "best slab (us)", "direct 128x128 / 64x64 (us)"))
    for n in (int(v) for v in a.batches.split(",")):
        for name, H, W, cin, cout, k, s in LAYERS:
            p = k // 2
            Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
            x = torch.randn(n, H, W, cin, device=dev).bfloat16()
            dy = (torch.randn(n, Ho, Wo, cout, device=dev) * 0.1).bfloat16()
            g = CL.geom_single(n, H, W, Ho, Wo, k, s, (p, p, p, p), cin, cout)
            out = torch.zeros(cout, k, k, cin, device=dev)
            flat = out.view(-1)
            slab = {}
            for v in list(CW._WGRAD_TILE) + list(CW._WGRAD_PIPE_TILE) + list(CW._WGRAD_P8):
                slab["hip%d" % v] = timeit(lambda v=v: CW.conv_wgrad(x, dy, g, None, out=flat, accumulate=True, variant=v),
                                           a.reps, a.inner)
            if CW.whalo_covers(g):
                slab["whalo"] = timeit(lambda: CW.halo_wgrad(x, dy, g, out=out, accumulate=True), a.reps, a.inner)
            direct = [timeit(lambda v=v: CW.conv_wgrad(x, dy, g, None, out=flat, accumulate=True, variant=v), a.reps, a.inner)
                      for v in CW._WGRAD_DIRECT]
            best = min(slab, key=slab.get)
            K = k * k * cin
            tiles = -(-K // 64) * -(-cout // 64)
            print("%-24s %2d %6d %5d  %-7s %7.1f  %s   %.2f" % (
                name, n, n * Ho * Wo, tiles, best, 1e3 * slab[best], " / ".join("%7.1f" % (1e3 * t) for t in direct),
                slab[best] / min(direct)), flush=True)


if __name__ == "__main__":
    main()
