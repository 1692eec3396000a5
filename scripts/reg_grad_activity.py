"""How sparse is the regression tower's gradient?  CPU only.

For bench.py's synthetic batches (16 x 800 x 1333, 1..20 boxes per image): M0 = the packed pyramid rows with at least
one positive anchor, Mk = M0 dilated k times by 3x3 per level (ops/halo.py), and for each the share of rows, of halo
tiles whose box + halo meets it (the data gradient's work items) and of 64-row K-tiles with a set row (the
phase-pipelined weight gradient's), and of halo tiles whose own pixels meet it (the un-extended rule: the FORWARD's
work items of the layer whose output is needed on Mk -- M0: the final, Mk: the tower layer k below it).
profiles/sparse_reg_grad.txt and profiles/sparse_reg_fwd.txt hold runs.

    python scripts/reg_grad_activity.py [--batches 4]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import anchors as A  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import halo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    a = ap.parse_args()
    N, H, W = a.batch_size, a.height, a.width
    shapes = [tuple(s) for s in A.guess_shapes((H, W))]
    nA = A.AnchorParameters.default.num_anchors()
    anchors = torch.from_numpy(A.anchors_for_shape((H, W)).astype(np.float32))
    tab = halo.build_tiles(N, shapes)
    P = N * sum(h * w for h, w in shapes)
    print("levels {}  rows {}  halo tiles {}  K-tiles {}".format(shapes, P, len(tab), (P + 63) // 64))
    stats = np.zeros((a.batches, 5, 4))
    for bi in range(a.batches):
        b = make_batch(N, H, W, generator=torch.Generator().manual_seed(bi))
        rows = np.zeros(P, dtype=bool)
        for i in range(N):      # image by image: the (A, G) IoU matrix of one image at a time
            state, _, _ = A.anchor_targets_torch(anchors, b["gt"][i:i + 1], b["gt_count"][i:i + 1],
                                                 b["image_hw"][i:i + 1])
            rows[i * (P // N):(i + 1) * (P // N)] = (state[0] == 1).reshape(-1, nA).any(dim=1).numpy()
        for k in range(5):
            words = halo.pack_row_bits(rows)
            stats[bi, k] = (rows.mean(), halo.active_tiles(tab, rows).mean(), (words != 0).mean(),
                            halo.active_tiles(tab, rows, ext=0).mean())
            rows = halo.dilate_rows(rows, N, shapes)
    print("{:<6}{:>16}{:>22}{:>22}{:>24}".format("mask", "rows non-zero", "halo tiles active", "64-row K-tiles active",
                                                 "forward tiles (un-ext)"))
    for k in range(5):
        lo, hi = 100 * stats[:, k].min(axis=0), 100 * stats[:, k].max(axis=0)
        print("M{:<5}{:>16}{:>22}{:>22}{:>24}".format(k, *("{:.1f}-{:.1f} %".format(l, h) for l, h in zip(lo, hi))))


if __name__ == "__main__":
    main()
