"""Timing of the BatchNorm + ReLU6 kernels (csrc/kernels/batch_norm.hip) on the distinct (n, C) forms of MobileNet-1.0's
27 norms in an 800 x 1333, batch-16 training step, against the form they replace: F.batch_norm + F.relu6 + autograd on
the channels-last NCHW view of the same NHWC bf16 tensor.  Forward (statistics, running update, apply) and backward
(dgamma, dbeta, dx) are timed apart; the two forms alternate within each of ROUNDS rounds of CALLS calls after a
warm-up.  Next to each kernel time stands the rate of the bytes of the fewest passes (forward: x twice, y once;
backward: dy and x twice, dx once), to be read against the 5.0 to 6.0 TB/s of profiles/r5_hbm_bw_probe.txt, and the
spread (max - min) / median of the rounds of both forms.  The first line lists which backend each norm of
models.backbone("mobilenet224_1.0").retinanet(80) takes on this device under bn_backend = "auto".
python scripts/bench_batchnorm.py [--batch 16] [--out FILE]"""
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

ROUNDS, CALLS = 5, 20
EPS, MOM = 1e-3, 0.01


def norm_forms(H, W):
    """{(H, W, C): [layer names]} of MobileNet-1.0's norms on an H x W image, in forward order."""
    H, W, C = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1, 32       # conv1: pad bottom / right, 3x3 valid, stride 2
    forms = {(H, W, C): ["conv1_bn"]}
    for i, (s, f) in enumerate(zip(MobileNet.STRIDES, MobileNet.FILTERS)):
        _, _, H, W = N.dwconv_geometry(H, W, s)
        forms.setdefault((H, W, C), []).append("conv_dw_{}_bn".format(i + 1))
        forms.setdefault((H, W, f), []).append("conv_pw_{}_bn".format(i + 1))
        C = f
    return forms


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
    net.bn_backend = "auto"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        net(torch.randn(2, 256, 320, 3, device=dev).bfloat16())
    return "mobilenet224_1.0 norms 1..27 backends (bf16, training, no warning raised): " + " ".join(net.bn_taken)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/batchnorm.txt)")
    args = ap.parse_args()
    N.load(required=True)
    dev = torch.device("cuda:0")
    B = args.batch
    lines = [backends_line(dev),
             "batch norm + ReLU6, training, NHWC bf16, batch {} of 800 x 1333 through MobileNet-1.0; {} rounds x {} calls, "
             "forms alternated; median us per call (min .. max of the rounds); TB/s = bytes of the fewest passes / native "
             "time; spread = (max - min) / median, the larger of the two forms".format(B, ROUNDS, CALLS)]
    g = torch.Generator(device=dev).manual_seed(1)
    for (H, W, C), layers in norm_forms(800, 1333).items():
        x = torch.randn(B, H, W, C, device=dev, generator=g).bfloat16().requires_grad_()
        dy = torch.randn(B, H, W, C, device=dev, generator=g).bfloat16()
        gamma = (2 + 0.25 * torch.randn(C, device=dev, generator=g)).requires_grad_()
        beta = (3 + 0.5 * torch.randn(C, device=dev, generator=g)).requires_grad_()
        rmean, rvar = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        xd, gd, bd = x.detach(), gamma.detach(), beta.detach()

        def torch_fwd(inp=xd, ga=gd, be=bd):
            return F.relu6(F.batch_norm(inp.permute(0, 3, 1, 2), rmean, rvar, ga, be, True, MOM, EPS))

        def native_fwd():
            mean, rstd = N.bn_stats(xd, rmean, rvar, True, MOM, EPS)
            return N.bn_act_fwd(xd, gd, bd, mean, rstd), mean, rstd

        yt, dyt = torch_fwd(x, gamma, beta), dy.permute(0, 3, 1, 2)      # the graph is kept for the backward
        _, mean, rstd = native_fwd()
        calls = {"fwd": (native_fwd, torch_fwd, 3),
                 "bwd": (lambda: N.bn_act_bwd(dy, xd, gd, bd, mean, rstd, True),
                         lambda: torch.autograd.grad(yt, (x, gamma, beta), dyt, retain_graph=True), 5)}
        lines.append("{} .. ({} norm{}): n = {} x {} x {} = {}, C = {}".format(
            layers[0], len(layers), "s" if len(layers) > 1 else "", B, H, W, B * H * W, C))
        for kind, (nat, ref, passes) in calls.items():
            for _ in range(3):
                nat(), ref()
            torch.cuda.synchronize()
            us = {"native": [], "torch": []}
            for _ in range(ROUNDS):
                us["native"].append(timed(nat))
                us["torch"].append(timed(ref))
            mn, mt = float(np.median(us["native"])), float(np.median(us["torch"]))
            spread = max((max(v) - min(v)) / float(np.median(v)) for v in us.values())
            lines.append("  {:<4} native {:8.1f} us ({:8.1f} .. {:8.1f})  {:5.2f} TB/s   torch {:8.1f} us ({:8.1f} .. {:8.1f})"
                         "   {:5.2f}x   spread {:4.1f} %".format(kind, mn, min(us["native"]), max(us["native"]),
                                                                 passes * 2 * B * H * W * C / mn * 1e-6, mt,
                                                                 min(us["torch"]), max(us["torch"]), mt / mn, 100 * spread))
        del x, dy, yt, dyt, calls
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
