"""Isolated timing of the distribution box head's kernels (csrc/kernels/box_dist.hip) at the bench shape: 16 images x
200,700 anchors, K = 17 bins per side (68 bf16 logits per row, 437 MB), ~1 % positive rows, the gradient written into
the packed regression final's padded rows (group 9, ld 640).  The two forms of the integral forward and the fused
DFL + backward alternated in one process, ROUNDS rounds of CALLS calls each after a warm-up.
python scripts/bench_box_dist.py [--out profiles/box_dist.txt]
Prints, per kernel, the median us per call over the rounds, the spread between rounds, the bytes it has to move and
their rate, and the time those bytes take at 5.0 and 6.0 TB/s (the range of profiles/r5_hbm_bw_probe.txt)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402

ROUNDS, CALLS, GROUP, K, R = 7, 10, 9, 17, 8.0
LD = (GROUP * 4 * K + 63) // 64 * 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "box_dist.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, A = 16, 200700
    rows = B * A
    target = torch.randn(B, A, 4, device=dev) * 2
    u = torch.rand(B, A, device=dev)
    state = torch.where(u < 0.01, 1, torch.where(u < 0.3, -1, 0)).to(torch.int8)
    npos = (state == 1).sum().to(torch.int32).reshape(1)
    logits = torch.empty(B, A, 4 * K, dtype=torch.bfloat16, device=dev)
    for b in range(B):
        logits[b] = torch.randn(A, 4 * K, device=dev).bfloat16()
    dreg = (torch.randn(B, A, 4, device=dev) / max(1, int(npos.item()))).bfloat16()
    out = torch.zeros(rows // GROUP, LD, dtype=torch.bfloat16, device=dev)
    state0 = torch.where(state == 1, torch.zeros_like(state), state)
    calls = {
        "integral_all": lambda: N.box_integral_fwd(logits, K, R),
        "integral_pos": lambda: N.box_integral_fwd(logits, K, R, state=state),
        "dist_bwd": lambda: N.box_dist_fwd_bwd(logits, dreg, target, state, npos, K, R, 0.25, grad_out=out, group=GROUP),
        # the same launch with no positive row: the zero fill alone
        "dist_bwd_nopos": lambda: N.box_dist_fwd_bwd(logits, dreg, target, state0, npos, K, R, 0.25, grad_out=out,
                                                     group=GROUP),
    }
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
    p = int(npos.item())
    row_logits = 4 * K * 2
    nbytes = {
        "integral_all": rows * (row_logits + 8),                                  # logits in, deltas out
        "integral_pos": rows * (1 + 8) + p * row_logits,                          # state in, deltas out, positive logits
        "dist_bwd": rows * (1 + row_logits) + p * (row_logits + 8 + 16),          # state, gradient rows out; positives:
                                                                                  # logits, delta gradient, target
        "dist_bwd_nopos": rows * (1 + row_logits),
    }
    med = {k: float(np.median(v)) for k, v in us.items()}
    lines = ["box_dist.hip, {} x {} rows x 4 x {} bf16, {} positive ({:.2f} %), padded group {} ld {}; {} rounds x {} "
             "calls, alternated (launch + finalize launch + the wrapper's allocations included)".format(
                 B, A, K, p, 100.0 * p / rows, GROUP, LD, ROUNDS, CALLS)]
    for k in calls:
        lines.append("{:<14} median {:7.1f} us/call  rounds {:7.1f} .. {:7.1f} us  {:6.1f} MB  {:5.2f} TB/s  bytes alone "
                     "{:6.1f} us at 6.0 TB/s, {:6.1f} us at 5.0 TB/s: {:3.0f} % .. {:3.0f} % of that rate".format(
                         k, med[k], min(us[k]), max(us[k]), nbytes[k] / 1e6, nbytes[k] / med[k] / 1e6,
                         nbytes[k] / 6.0e6, nbytes[k] / 5.0e6, 100 * nbytes[k] / 6.0e6 / med[k],
                         100 * nbytes[k] / 5.0e6 / med[k]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
