"""Isolated timing of the fused regression loss + gradient kernels at the bench shape (16 images x 200,700 anchors,
bf16 deltas, ~1 % positive rows, the gradient written into the packed regression final's padded rows: group 9,
ld 64): smooth-L1 and the three IoU kinds alternated in one process, ROUNDS rounds of 20 calls each after a
warm-up.  python scripts/bench_iou_loss.py [--out profiles/iou_loss.txt]
Prints, per kernel, the median us per call over the rounds, the spread between rounds, the rate of the bytes it has
to move (the state read, the gradient write, and prediction + target + anchor of the positive rows) and the ratio
to smooth-L1."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops.anchors import anchors_for_shape  # noqa: E402

ROUNDS, CALLS, GROUP, LD = 7, 20, 9, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "iou_loss.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    anchors = torch.from_numpy(anchors_for_shape((800, 1333, 3)).astype(np.float32)).to(dev)
    B, A = 16, anchors.shape[0]
    assert A == 200700
    target = torch.randn(B, A, 4, device=dev) * 0.5
    pred = (target + torch.randn(B, A, 4, device=dev)).bfloat16()
    u = torch.rand(B, A, device=dev)
    state = torch.where(u < 0.01, 1, torch.where(u < 0.3, -1, 0)).to(torch.int8)
    npos = (state == 1).sum().to(torch.int32).reshape(1)
    out = torch.zeros(B * A // GROUP, LD, dtype=torch.bfloat16, device=dev)
    calls = {"smooth_l1": lambda: N.smooth_l1_fwd_bwd(pred, target, state, npos, grad_out=out, group=GROUP)}
    for kind in ("giou", "diou", "ciou"):
        calls[kind] = lambda kind=kind: N.iou_loss_fwd_bwd(pred, target, anchors, state, npos, kind=kind, grad_out=out,
                                                           group=GROUP)
    for f in calls.values():
        for _ in range(3):
            f()
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
    rows, p = B * A, int(npos.item())
    base = rows * (1 + 4 * 2)                     # state in, bf16 gradient out
    nbytes = {k: base + p * (4 * 2 + 4 * 4 + (0 if k == "smooth_l1" else 4 * 4)) for k in calls}
    med = {k: float(np.median(v)) for k, v in us.items()}
    lines = ["regression loss kernels, {} x {} rows bf16, {} positive ({:.2f} %), padded group {} ld {}; {} rounds x {} "
             "calls, alternated (launch + finalize launch + the wrapper's two allocations included)".format(
                 B, A, p, 100.0 * p / rows, GROUP, LD, ROUNDS, CALLS)]
    for k in calls:
        lines.append("{:<10} median {:7.1f} us/call  rounds {:7.1f} .. {:7.1f} us  {:5.2f} TB/s  {:.3f} x smooth_l1".format(
            k, med[k], min(us[k]), max(us[k]), nbytes[k] / med[k] / 1e6, med[k] / med["smooth_l1"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
