"""Timing of the depthwise 3x3 kernels (csrc/kernels/dwconv.hip) on the depthwise layers of MobileNet-1.0 in an
800 x 1333, batch-16 step, against the form they replace: F.pad + F.conv2d(groups=C) + autograd on the NCHW view of the
same NHWC tensor.  Per layer form, forward, data gradient and weight gradient are timed apart; the two forms alternate
within each of ROUNDS rounds of CALLS calls after a warm-up.  Next to each kernel time stands the rate of the bytes the
operation needs (both activations once; the taps are noise), to be read against the 5.0 to 6.0 TB/s of
profiles/r5_hbm_bw_probe.txt.  The first line lists which backend each conv_dw layer of
models.backbone("mobilenet224_1.0").retinanet(80) takes on this device.
python scripts/bench_dwconv.py [--batch 16] [--out FILE]"""
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
from batchai_retinanet_horovod_coco_amd.ops import depthwise as D  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402

ROUNDS, CALLS = 5, 20


def layer_forms(H, W):
    """(first layer, layers, H, W, C, stride) per distinct depthwise form of MobileNet-1.0 on an H x W image."""
    H, W, C = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1, 32       # conv1: pad bottom / right, 3x3 valid, stride 2
    forms = {}
    for i, (s, f) in enumerate(zip(MobileNet.STRIDES, MobileNet.FILTERS)):
        forms.setdefault((H, W, C, s), []).append(i + 1)
        _, _, H, W = N.dwconv_geometry(H, W, s)
        C = f
    return [(v, k) for k, v in forms.items()]


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(CALLS):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / CALLS * 1e3      # us per call


def backends_line(dev):
    model = models.backbone("mobilenet224_1.0").retinanet(80).to(dev)
    net = next(m for m in model.modules() if isinstance(m, MobileNet))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        net(torch.randn(2, 256, 320, 3, device=dev).bfloat16())
    return "mobilenet224_1.0 conv_dw_1..13 backends (bf16, no warning raised): " + " ".join(net.dw_taken)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/dwconv.txt)")
    args = ap.parse_args()
    N.load(required=True)
    dev = torch.device("cuda:0")
    B = args.batch
    lines = [backends_line(dev),
             "depthwise 3x3, NHWC bf16, batch {} of 800 x 1333 through MobileNet-1.0; {} rounds x {} calls, forms "
             "alternated; median us per call (min .. max of the rounds); TB/s = bytes needed / native time"
             .format(B, ROUNDS, CALLS)]
    g = torch.Generator(device=dev).manual_seed(1)
    for layers, (H, W, C, s) in layer_forms(800, 1333):
        x = torch.randn(B, H, W, C, device=dev, generator=g).bfloat16().requires_grad_()
        w = torch.randn(C, 1, 3, 3, device=dev, generator=g).requires_grad_()
        wb = w.detach().bfloat16().requires_grad_()
        _, _, Ho, Wo = N.dwconv_geometry(H, W, s)
        dy = torch.randn(B, Ho, Wo, C, device=dev, generator=g).bfloat16()
        w9 = N.dwconv_taps(w)
        xd = x.detach()
        yt = D.depthwise_conv3x3_torch(x, wb, s)      # the parent's form; its graph is kept for the two gradients
        calls = {
            "fwd": (lambda: N.dwconv3x3_fwd(xd, w9, s), lambda: D.depthwise_conv3x3_torch(xd, wb.detach(), s)),
            "dgrad": (lambda: N.dwconv3x3_dgrad(dy, w9, xd.shape, s),
                      lambda: torch.autograd.grad(yt, x, dy, retain_graph=True)),
            "wgrad": (lambda: N.dwconv3x3_wgrad(dy, xd, s), lambda: torch.autograd.grad(yt, wb, dy, retain_graph=True)),
        }
        nbytes = 2 * C * B * (H * W + Ho * Wo)
        lines.append("conv_dw_{} ({} layer{}): {} x {} x {}, stride {}".format(
            layers[0], len(layers), "s" if len(layers) > 1 else "", H, W, C, s))
        for kind, (nat, ref) in calls.items():
            for _ in range(3):
                nat(), ref()
            torch.cuda.synchronize()
            us = {"native": [], "torch": []}
            for _ in range(ROUNDS):
                us["native"].append(timed(nat))
                us["torch"].append(timed(ref))
            mn, mt = float(np.median(us["native"])), float(np.median(us["torch"]))
            lines.append("  {:<5} native {:8.1f} us ({:8.1f} .. {:8.1f})  {:5.2f} TB/s   torch {:8.1f} us ({:8.1f} .. {:8.1f})"
                         "   {:5.2f}x".format(kind, mn, min(us["native"]), max(us["native"]), nbytes / mn * 1e-6, mt,
                                              min(us["torch"]), max(us["torch"]), mt / mn))
        del x, w, wb, dy, yt, calls
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
