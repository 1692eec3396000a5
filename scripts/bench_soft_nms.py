"""Timing of the batched device FilterDetections with hard NMS (csrc/kernels/filter.hip) and with the two Soft-NMS kinds
(csrc/kernels/soft_nms.hip) on two inputs: the production batch of test_batched_filter_production_batch_time (B = 16,
200,700 anchors, 80 classes, ~100 candidates per (image, class)) and a crowded one (~2,000 per segment).  The kinds are
alternated in one process, ROUNDS rounds of CALLS calls each after a warm-up; a call is the whole wrapper (select, the
per-segment stage, the overflow check's host sync, the top-k).
python scripts/bench_soft_nms.py [--kinds hard,linear,gaussian] [--tree DIR --label NAME] [--out FILE]
--tree DIR imports the package from another checkout (the parent commit's, built, with --kinds hard) so that both run
on one box in one job."""
import argparse
import os
import sys

import numpy as np
import torch

ROUNDS, CALLS = 7, 50
INPUTS = (("production", 0.0005), ("crowded", 0.012))


def make_inputs(dev, B, A, C, H, W, hot, seed=5, cold=-8.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ctr = torch.rand(A, 2, device=dev, generator=g) * torch.tensor([W, H], device=dev)
    wh = 16 + torch.rand(A, 2, device=dev, generator=g) * 200
    anchors = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    deltas = (torch.randn(B, A, 4, device=dev, generator=g) * 0.5).bfloat16()
    logits = torch.randn(B, A, C, device=dev, generator=g) + cold
    hotm = torch.rand(B, A, C, device=dev, generator=g) < hot
    return anchors, deltas, torch.where(hotm, logits + 6.0, logits).bfloat16()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="hard,linear,gaussian")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=None, help="also write the report here (profiles/soft_nms.txt joins three runs)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    N.load(required=True)
    dev = torch.device("cuda:0")
    kinds = args.kinds.split(",")
    B, A, C, H, W, D = 16, 200700, 80, 800.0, 1333.0, 300
    lines = ["filter_detections_batched, B = {} x {} anchors x {} classes bf16, max_detections {}, {}; {} rounds x {} "
             "calls, kinds alternated; ms per call".format(B, A, C, D, args.label, ROUNDS, CALLS)]
    for name, hot in INPUTS:
        anchors, deltas, logits = make_inputs(dev, B, A, C, H, W, hot)
        per_seg = (torch.sigmoid(logits.float()) > 0.05).sum(1).float()
        calls = {k: (lambda k=k: N.filter_detections_batched(anchors, deltas, logits, H, W,
                                                             **({} if k == "hard" else {"nms_kind": k})))
                 for k in kinds}
        kept = {}
        for k, f in calls.items():
            for _ in range(2):
                kept[k] = int((f()[1] >= 0).sum())
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, f in calls.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                for _ in range(CALLS):
                    f()
                ev[1].record()
                torch.cuda.synchronize()
                ms[k].append(ev[0].elapsed_time(ev[1]) / CALLS)
        lines.append("{}: candidates per (image, class) mean {:.0f}, max {:.0f}".format(name, float(per_seg.mean()),
                                                                                       float(per_seg.max())))
        base = float(np.median(ms[kinds[0]]))
        for k in kinds:
            med = float(np.median(ms[k]))
            lines.append("  {:<9} median {:8.3f} ms  rounds {:8.3f} .. {:8.3f} ms  {:+8.3f} ms over {}  detections kept {}"
                         .format(k, med, min(ms[k]), max(ms[k]), med - base, kinds[0], kept[k]))
        del anchors, deltas, logits, calls
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
