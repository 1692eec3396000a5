"""Timing of the pointwise 1x1 kernels (csrc/kernels/pwconv.hip) on the conv_pw layers of MobileNet-1.0 in an
800 x 1333, batch-16 step, against the form they replace: F.conv2d + autograd on the channels-last bf16 view of the same
tensor, and -- where Cin % 64 == 0 -- against the project's ResNet conv front-end, native_conv.conv2d.  Per layer form,
forward, data gradient and weight gradient are timed apart; the forms alternate within each of ROUNDS rounds of CALLS
calls after a warm-up.  Next to each kernel time stand the rate of the bytes the operation needs (both activations once;
the weight is noise), to be read against the 5.0 to 6.0 TB/s of profiles/r5_hbm_bw_probe.txt, and the TF/s of its
2 M Ci Co flops.  The first line lists which backend each conv_pw layer of
models.backbone("mobilenet224_1.0").retinanet(80) takes under pw_backend = "auto" on this device.
python scripts/bench_pwconv.py [--batch 16] [--out FILE]"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd import models  # noqa: E402
from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native_conv  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import pointwise as P  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops.conv_launch import hip_conv_ok  # noqa: E402

ROUNDS, CALLS = 5, 10


def layer_forms(H, W):
    """(layers, (H, W, Ci, Co)) per distinct pointwise form of MobileNet-1.0 on an H x W image."""
    H, W, C = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1, 32       # conv1: pad bottom / right, 3x3 valid, stride 2
    forms = {}
    for i, (s, f) in enumerate(zip(MobileNet.STRIDES, MobileNet.FILTERS)):
        _, _, H, W = N.dwconv_geometry(H, W, s)
        forms.setdefault((H, W, C, f), []).append(i + 1)
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
    net.pw_backend = "auto"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        net(torch.randn(2, 256, 320, 3, device=dev).bfloat16())
    return ("mobilenet224_1.0 conv_pw_1..13 backends under pw_backend = 'auto' (bf16, no warning raised): "
            + " ".join(net.pw_taken))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/pwconv.txt)")
    args = ap.parse_args()
    N.load(required=True)
    dev = torch.device("cuda:0")
    B = args.batch
    lines = [backends_line(dev),
             "pointwise 1x1, NHWC bf16, batch {} of 800 x 1333 through MobileNet-1.0; {} rounds x {} calls, forms "
             "alternated; median us per call (min .. max of the rounds); TB/s = bytes needed / native time, TF/s = "
             "2 M Ci Co / native time; 'conv' = native_conv.conv2d".format(B, ROUNDS, CALLS)]
    g = torch.Generator(device=dev).manual_seed(1)
    total = {}
    for layers, (H, W, ci, co) in layer_forms(800, 1333):
        x = torch.randn(B, H, W, ci, device=dev, generator=g).bfloat16().requires_grad_()
        wb = torch.randn(co, ci, 1, 1, device=dev, generator=g).bfloat16().requires_grad_()
        dy = torch.randn(B, H, W, co, device=dev, generator=g).bfloat16()
        xd, w2 = x.detach(), N.pwconv_weight(wb)
        yt = P.pointwise_conv_torch(x, wb)            # the parent's form; its graph is kept for the two gradients
        calls = {"fwd": [lambda: N.pwconv_fwd(xd, w2), lambda: P.pointwise_conv_torch(xd, wb.detach())],
                 "dgrad": [lambda: N.pwconv_dgrad(dy, w2), lambda: torch.autograd.grad(yt, x, dy, retain_graph=True)],
                 "wgrad": [lambda: N.pwconv_wgrad(dy, xd), lambda: torch.autograd.grad(yt, wb, dy, retain_graph=True)]}
        if hip_conv_ok(ci, co, x.dtype):
            wo = wb.detach().reshape(co, 1, 1, ci)    # OHWI
            wr = wo.clone().requires_grad_()
            yx = native_conv.conv2d(x, wo, None, 1, (0, 0, 0, 0), False, None)
            yw = native_conv.conv2d(xd, wr, None, 1, (0, 0, 0, 0), False, None)
            calls["fwd"].append(lambda: native_conv.conv2d(xd, wo, None, 1, (0, 0, 0, 0), False, None))
            calls["dgrad"].append(lambda: torch.autograd.grad(yx, x, dy, retain_graph=True))
            calls["wgrad"].append(lambda: torch.autograd.grad(yw, wr, dy, retain_graph=True))
        m = B * H * W
        nbytes, flops = 2 * m * (ci + co), 2 * m * ci * co
        lines.append("conv_pw_{} ({} layer{}): M = {} ({} x {}), {} -> {}, {:.0f} flops per byte".format(
            layers[0], len(layers), "s" if len(layers) > 1 else "", m, H, W, ci, co, flops / nbytes))
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
            for k, t in enumerate(med[:2]):
                total[(layers[0], k)] = total.get((layers[0], k), 0.0) + t
            line = "  {:<5} native {:8.1f} us ({:8.1f} .. {:8.1f})  {:5.2f} TB/s {:6.1f} TF/s   torch {:8.1f} us ({:8.1f} .. " \
                   "{:8.1f})  {:5.2f}x".format(kind, med[0], min(us[0]), max(us[0]), nbytes / med[0] * 1e-6,
                                               flops / med[0] * 1e-6, med[1], min(us[1]), max(us[1]), med[1] / med[0])
            if len(fns) > 2:
                line += "   conv {:8.1f} us ({:8.1f} .. {:8.1f})  {:5.2f}x".format(med[2], min(us[2]), max(us[2]),
                                                                                 med[2] / med[0])
            lines.append(line)
        lines.append("  fwd + dgrad + wgrad: native {:8.1f} us, torch {:8.1f} us, {:5.2f}x".format(
            total[(layers[0], 0)], total[(layers[0], 1)], total[(layers[0], 1)] / total[(layers[0], 0)]))
        del x, wb, dy, yt, calls
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
