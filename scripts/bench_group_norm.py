"""Isolated timing of the fused GroupNorm + ReLU kernels (group_norm.hip) at the bench shape: 16 images, levels
[(100,167),(50,84),(25,42),(13,21),(7,11)] packed [16, 22300, 256] bf16, 32 groups.  The new forward + backward is
alternated in one process with what a user has today: F.group_norm + relu per level on views of the packed tensor,
forward + backward.  python scripts/bench_group_norm.py [--out profiles/group_norm_kernels.txt]   (section 1 of
profiles/group_norm.txt is a copy of that file; its other sections are step measurements this script does not make)
Prints, per arm, the median us per forward + backward over the rounds and the spread between rounds; for the kernels
also the forward and the backward on their own, the rate of the bytes they have to move (3 x the tensor forward, 5 x
backward, plus the statistics) and its share of the 5.0 to 6.0 TB/s profiles/r5_hbm_bw_probe.txt measured."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402

ROUNDS, CALLS = 7, 10
B, C, G, EPS = 16, 256, 32, 1e-5
SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21), (7, 11)]


def timed(f):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(CALLS):
        f()
    ev[1].record()
    torch.cuda.synchronize()
    return 1e3 * ev[0].elapsed_time(ev[1]) / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "group_norm_kernels.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    P = sum(h * w for h, w in SHAPES)
    x = (torch.randn(B, P, C, device=dev) * 1.5 + 0.3).bfloat16()
    dy = torch.randn(B, P, C, device=dev).bfloat16()
    gamma = (1 + 0.1 * torch.randn(C, device=dev)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, device=dev)).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    saved = {}

    def fwd():
        saved["s"] = N.gn_relu_fwd(x, SHAPES, gamma.detach(), beta.detach(), G, EPS)

    def bwd():
        _, mean, rstd = saved["s"]
        N.gn_relu_bwd(dy, x, SHAPES, gamma.detach(), beta.detach(), mean, rstd, G)

    def both():
        fwd()
        bwd()

    def torch_both():
        xg.grad = gamma.grad = beta.grad = None
        out, off = [], 0
        for h, w in SHAPES:
            lv = xg[:, off:off + h * w].reshape(B, h, w, C).permute(0, 3, 1, 2)
            out.append(torch.relu(F.group_norm(lv, G, gamma.to(lv.dtype), beta.to(lv.dtype), EPS))
                       .permute(0, 2, 3, 1).reshape(B, h * w, C))
            off += h * w
        torch.cat(out, 1).backward(dy)

    calls = {"hip fwd+bwd": both, "torch fwd+bwd": torch_both, "hip fwd": fwd, "hip bwd": bwd}
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, f in calls.items():
            us[k].append(timed(f))
    tensor, stats = B * P * C * 2, 2 * B * len(SHAPES) * G * 4
    nbytes = {"hip fwd": 3 * tensor + stats, "hip bwd": 5 * tensor + stats + 2 * C * 4}
    nbytes["hip fwd+bwd"] = nbytes["hip fwd"] + nbytes["hip bwd"]
    med = {k: float(np.median(v)) for k, v in us.items()}
    lines = ["GroupNorm + ReLU, {} x {} x {} bf16 ({:.1f} MB), {} groups, levels {}; {} rounds x {} calls, alternated "
             "(the wrapper's allocations included)".format(B, P, C, tensor / 1e6, G, SHAPES, ROUNDS, CALLS)]
    for k in calls:
        line = "{:<14} median {:8.1f} us  rounds {:8.1f} .. {:8.1f} us".format(k, med[k], min(us[k]), max(us[k]))
        if k in nbytes:
            rate = nbytes[k] / med[k] / 1e6
            line += "  {:5.2f} TB/s of the bytes needed ({:.0f} % / {:.0f} % of 5.0 / 6.0 TB/s)".format(
                rate, 100 * rate / 5.0, 100 * rate / 6.0)
        lines.append(line)
    spread = max(max(us[k]) - min(us[k]) for k in ("hip fwd+bwd", "torch fwd+bwd"))
    lines.append("torch / hip {:.2f} x; the kernels are {:.1f} us faster, the larger spread of the two arms is {:.1f} us"
                 .format(med["torch fwd+bwd"] / med["hip fwd+bwd"], med["torch fwd+bwd"] - med["hip fwd+bwd"], spread))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
