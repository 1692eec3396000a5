"""Timing of the stem kernels (csrc/kernels/stem3x3.hip) on MobileNet's conv1 in an 800 x 1333, batch-16 step, for
Co = 8, 16, 24, 32 (alpha 0.25 .. 1.0), against the form they replace: F.pad + F.conv2d on the NCHW view + the
channels-last copy of the result, and autograd's weight gradient of that.  Forward (weight pack included) and weight
gradient are timed apart; the forms alternate within each of ROUNDS rounds of CALLS calls after a warm-up.  Next to each
kernel time stands the rate of the bytes the operation needs (image and output activation once; the weight is noise),
to be read against the 5.0 to 6.0 TB/s of profiles/r5_hbm_bw_probe.txt.  The first line says which path conv1 of
models.backbone("mobilenet224_1.0").retinanet(80) takes under stem_backend = "auto" on this device.
python scripts/bench_stem3x3.py [--batch 16] [--out FILE]"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd import models  # noqa: E402
from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402

ROUNDS, CALLS = 5, 10


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(CALLS):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / CALLS * 1e3      # us per call


def torch_form(x, w):
    """What MobileNet.forward does for conv1 under stem_backend = 'torch' in front of the native batch-norm."""
    y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)), w, stride=2)
    return y.contiguous(memory_format=torch.channels_last)


def backend_line(dev):
    model = models.backbone("mobilenet224_1.0").retinanet(80).to(dev)
    net = next(m for m in model.modules() if isinstance(m, MobileNet))
    net.stem_backend = "auto"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        net(torch.randn(2, 256, 320, 3, device=dev).bfloat16())
    return "mobilenet224_1.0 conv1 under stem_backend = 'auto' (bf16, no warning raised): " + net.stem_taken


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/stem3x3.txt)")
    args = ap.parse_args()
    N.load(required=True)
    dev = torch.device("cuda:0")
    B, H, W = args.batch, 800, 1333
    _, _, Ho, Wo = N.dwconv_geometry(H, W, 2)
    lines = [backend_line(dev),
             "stem 3x3 / s2, NHWC bf16, batch {} of {} x {} x 3 -> {} x {} x Co; {} rounds x {} calls, forms alternated; "
             "median us per call (min .. max of the rounds); TB/s = bytes needed / native time; 'torch' = pad + conv2d + "
             "channels-last copy, and autograd's weight gradient of it".format(B, H, W, Ho, Wo, ROUNDS, CALLS)]
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, H, W, 3, device=dev, generator=g).bfloat16()
    for co in (8, 16, 24, 32):
        wb = torch.randn(co, 3, 3, 3, device=dev, generator=g).bfloat16().requires_grad_()
        wd = wb.detach()
        dy = torch.randn(B, Ho, Wo, co, device=dev, generator=g).bfloat16()
        dyc = dy.permute(0, 3, 1, 2)
        yt = torch_form(x, wb)                        # the parent's form; its graph is kept for the weight gradient
        calls = {"fwd": [lambda: N.stem3_fwd(x, N.stem3_weight(wd), co), lambda: torch_form(x, wd)],
                 "wgrad": [lambda: N.stem3_wgrad(dy, x), lambda: torch.autograd.grad(yt, wb, dyc, retain_graph=True)]}
        nbytes = 2 * (x.numel() + dy.numel())
        lines.append("Co = {}: M = {} pixels, {:.1f} MB needed".format(co, B * Ho * Wo, nbytes * 1e-6))
        total = [0.0, 0.0]
        for kind, fns in calls.items():
            for _ in range(2):
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
            us = [[] for _ in fns]
            for _ in range(ROUNDS):
                for u, fn in zip(us, fns):
                    u.append(timed(fn))
            med = [float(np.median(u)) for u in us]
            total = [t + m for t, m in zip(total, med)]
            lines.append("  {:<5} native {:8.1f} us ({:8.1f} .. {:8.1f})  {:5.2f} TB/s   torch {:8.1f} us ({:8.1f} .. {:8.1f})  "
                         "{:5.2f}x".format(kind, med[0], min(us[0]), max(us[0]), nbytes / med[0] * 1e-6, med[1], min(us[1]),
                                           max(us[1]), med[1] / med[0]))
        lines.append("  fwd + wgrad: native {:8.1f} us, torch {:8.1f} us, {:5.2f}x".format(total[0], total[1],
                                                                                         total[1] / total[0]))
        del wb, dy, dyc, yt, calls
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
