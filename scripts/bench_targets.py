"""Isolated timing of the two anchor-target assigners at the bench shape (16 images x the 200,700 anchors of a padded
800 x 1333 image; 20 and 100 boxes per image, sizes log-uniform between 16 px and 60 % of the short side as the
synthetic COCO-shaped batches draw them): the fixed-threshold kernel and ATSS (topk 9) alternated in one process,
ROUNDS rounds of 200 calls each after a warm-up.  python scripts/bench_targets.py [--out profiles/atss_targets.txt]
Prints, per assigner and box count, the median us per call over the rounds, the spread between rounds, the share of
a 30 ms training step, the number of positives it assigns and, for ATSS, the ratio to the fixed-threshold kernel."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd.ops import anchors as A  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402

ROUNDS, CALLS, STEP_MS, H, W, B = 7, 200, 30.0, 800, 1333, 16


def boxes(n, dev):
    """(B, n, 5) boxes drawn as data.synthetic.make_batch draws them, every row valid; counts; image sizes."""
    g = torch.Generator().manual_seed(n)
    lo, hi = math.log(16.0), math.log(0.6 * min(H, W))
    wh = torch.exp(lo + (hi - lo) * torch.rand((B, n, 2), generator=g))
    ar = torch.exp((torch.rand((B, n, 1), generator=g) - 0.5) * 1.4)
    w, h = (wh[..., 0:1] * ar).clamp(max=W - 2), (wh[..., 1:2] / ar).clamp(max=H - 2)
    x1, y1 = torch.rand((B, n, 1), generator=g) * (W - 1 - w), torch.rand((B, n, 1), generator=g) * (H - 1 - h)
    gt = torch.cat([x1, y1, x1 + w, y1 + h, torch.randint(0, 80, (B, n, 1), generator=g).float()], -1)
    return (gt.to(dev), torch.full((B,), n, dtype=torch.int32, device=dev),
            torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "atss_targets.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    a64 = A.anchors_for_shape((H, W, 3))
    anchors = torch.from_numpy(a64.astype(np.float32)).to(dev)
    centers = torch.from_numpy(A.centers_round_down(a64)).to(dev)
    levels = A.level_table((H, W))
    assert anchors.shape[0] == 200700
    calls, npos = {}, {}
    for n in (20, 100):
        gt, cnt, hw = boxes(n, dev)
        calls[("iou", n)] = lambda gt=gt, cnt=cnt, hw=hw: N.anchor_targets(anchors, gt, cnt, hw, centers=centers)
        calls[("atss", n)] = lambda gt=gt, cnt=cnt, hw=hw: N.atss_targets(anchors, levels, gt, cnt, hw, topk=9,
                                                                          centers=centers)
    for k, f in calls.items():
        for _ in range(3):
            out = f()
        npos[k] = int(out[3].item())
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, f in calls.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(CALLS):
                f()
            ev[1].record()
            torch.cuda.synchronize()
            us[k].append(1e3 * ev[0].elapsed_time(ev[1]) / CALLS)
    med = {k: float(np.median(v)) for k, v in us.items()}
    lines = ["anchor targets, {} images x {} anchors (padded {} x {}), boxes 16 px .. 60 % of the short side; {} rounds x {} "
             "calls, alternated (every launch of the call and the wrapper's allocations included); share of a {:.0f} ms "
             "step".format(B, anchors.shape[0], H, W, ROUNDS, CALLS, STEP_MS)]
    for (kind, n) in calls:
        k = (kind, n)
        lines.append("{:<5} {:>3} boxes/image  median {:7.1f} us/call  rounds {:7.1f} .. {:7.1f} us  {:5.2f} % of the step  "
                     "{:>6} positives  {:.2f} x iou".format(kind, n, med[k], min(us[k]), max(us[k]),
                                                            100.0 * med[k] / (1e3 * STEP_MS), npos[k],
                                                            med[k] / med[("iou", n)]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
