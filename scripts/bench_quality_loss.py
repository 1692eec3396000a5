"""Isolated timing of the fused classification loss + gradient kernels at the bench shape (16 images x 200,700 anchors
x 80 classes, bf16 logits, ~1 % positive rows, the gradient written into the packed classification final's padded
rows: group 9, ld 768): focal, QFL and VFL alternated in one process, ROUNDS rounds of CALLS calls each after a
warm-up.  python scripts/bench_quality_loss.py [--out profiles/quality_loss.txt]
Prints, per kernel, the median us per call over the rounds, the spread between rounds, the rate of the bytes it has
to move (the logits read, the gradient write, state and label per row, and prediction + target + anchor of the
positive rows for QFL / VFL) and the ratio to focal.  A fourth line, qfl_nopos, is QFL on the same tensors with the
positive rows made negative: the kernel without its label branch."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops.anchors import anchors_for_shape  # noqa: E402

ROUNDS, CALLS, GROUP, LD, C = 7, 10, 9, 768, 80


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "quality_loss.txt"))
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
    label = torch.randint(0, C, (B, A), device=dev, dtype=torch.int32)
    npos = (state == 1).sum().to(torch.int32).reshape(1)
    logits = torch.empty(B, A, C, dtype=torch.bfloat16, device=dev)
    for b in range(B):      # a prior-initialised head a few steps in: logits around -4.6, inside focal's clip range
        logits[b] = (torch.randn(A, C, device=dev) - 4.6).bfloat16()
    out = torch.zeros(B * A // GROUP, LD, dtype=torch.bfloat16, device=dev)
    calls = {"focal": lambda: N.focal_fwd_bwd(logits, state, label, npos, grad_out=out, group=GROUP)}
    for kind in ("qfl", "vfl"):
        calls[kind] = lambda kind=kind: N.quality_loss_fwd_bwd(logits, pred, target, anchors, state, label, npos,
                                                               kind=kind, grad_out=out, group=GROUP)
    # the same launch with no positive row: what the label branch (its loads, the IoU, the library exp / log1p, in
    # a wave that waits for the one lane) costs is the difference to the line above it
    state0 = torch.where(state == 1, torch.zeros_like(state), state)
    calls["qfl_nopos"] = lambda: N.quality_loss_fwd_bwd(logits, pred, target, anchors, state0, label, npos, kind="qfl",
                                                        grad_out=out, group=GROUP)
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
    base = rows * (C * 2 * 2 + 1 + 4)             # bf16 logits in, bf16 gradient out, state, label
    nbytes = {k: base + (p * (4 * 2 + 4 * 4 + 4 * 4) if k in ("qfl", "vfl") else 0) for k in calls}
    med = {k: float(np.median(v)) for k, v in us.items()}
    lines = ["classification loss kernels, {} x {} rows x {} bf16, {} positive ({:.2f} %), padded group {} ld {}; {} "
             "rounds x {} calls, alternated (launch + finalize launch + the wrapper's two allocations included)".format(
                 B, A, C, p, 100.0 * p / rows, GROUP, LD, ROUNDS, CALLS)]
    for k in calls:
        lines.append("{:<9} median {:7.1f} us/call  rounds {:7.1f} .. {:7.1f} us  {:5.2f} TB/s  {:.3f} x focal".format(
            k, med[k], min(us[k]), max(us[k]), nbytes[k] / med[k] / 1e6, med[k] / med["focal"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
