"""Timing of the fused separable-block kernel (csrc/kernels/sepblock.hip) on the 13 blocks of MobileNet-1.0 in eval mode
at batch 16, 800 x 1333, bf16, against the two forms it can replace: the per-layer native chain (dwconv.hip,
batch_norm.hip, pwconv.hip, batch_norm.hip: ``dw_backend = bn_backend = pw_backend = "native"``) and the torch form
(all three ``"torch"``), both run through the backbone's own layer methods.  Per distinct block form the three
alternate within each of ROUNDS rounds of CALLS calls after a warm-up.  Where ``native.sepblock_form`` picks the stream
form (csrc/kernels/sepblock_stream.hip: blocks 7 to 13), both fused forms are timed, and the verdict is about the one
``auto`` would run.  Next to each time stands the rate of the bytes
the block must move (x once, y once; weights and vectors are noise), to be read against the 5.0 to 6.0 TB/s of
profiles/r5_hbm_bw_probe.txt.  A form whose fused time exceeds the better of the other two by more than the spread of
the rounds is marked LOSES: those are the forms for ``native.SEP_AUTO_EXCLUDED``.  Last, a whole eval forward of
MobileNet(1.0) is timed with ``block_backend = "native"`` and ``"auto"`` over the native layers (``auto`` also with
this run's losing forms and with every stream form excluded, the forward before the stream kernel), and as the native
layers and the torch layers alone.
python scripts/bench_sepblock.py [--batch 16] [--out FILE]   (profiles/sepblock.txt, profiles/sepblock_stream.txt)"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet, _autocast, _nchw  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import separable as SB  # noqa: E402

ROUNDS, CALLS = 5, 10


def block_forms(H, W):
    """(blocks, (H, W, Ci, Co, stride)) per distinct block form of MobileNet-1.0 on an H x W image."""
    H, W, C = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1, 32       # conv1: pad bottom / right, 3x3 valid, stride 2
    forms = {}
    for i, (s, f) in enumerate(zip(MobileNet.STRIDES, MobileNet.FILTERS)):
        forms.setdefault((H, W, C, f, s), []).append(i)
        _, _, H, W = N.dwconv_geometry(H, W, s)
        C = f
    return [(v, k) for k, v in forms.items()]


def timed(fn, calls=CALLS):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(calls):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / calls * 1e3      # us per call


def rounds(fns, calls=CALLS):
    """Median, min and max us per call of each function; the functions alternate within every round."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(ROUNDS):
        for u, fn in zip(us, fns):
            u.append(timed(fn, calls))
    return [(float(np.median(u)), min(u), max(u)) for u in us]


def set_layers(net, backend):
    net.dw_backend = net.bn_backend = net.pw_backend = backend


def randomise_statistics(net, g):
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, device=m.weight.device, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, device=m.weight.device, generator=g) * 3.75 + 0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/sepblock.txt)")
    args = ap.parse_args()
    N.load(required=True)
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(1)
    net = MobileNet(1.0).to(dev).eval()
    randomise_statistics(net, g)
    lines = ["separable block, eval mode, NHWC bf16, batch {} of 800 x 1333 through MobileNet-1.0; {} rounds x {} calls, "
             "forms alternated; median us per call (min .. max of the rounds); TB/s = (bytes of x + bytes of y) / time"
             .format(B, ROUNDS, CALLS)]
    losers = []
    with torch.no_grad():
        for blocks, (H, W, ci, co, s) in block_forms(800, 1333):
            i = blocks[0]
            xh = torch.randn(B, H, W, ci, device=dev, generator=g).bfloat16()
            x = _nchw(xh)
            ops = (xh, net.dw[i].weight, net.dw_bn[i].bn, net.pw[i].weight, net.pw_bn[i].bn, s)

            def layers(backend):
                set_layers(net, backend)
                with _autocast(x):
                    y = net.dw_bn[i](net._depthwise(i, x), backend)
                    return net.pw_bn[i](net._pointwise(i, y), backend)

            def fused_as(form):
                # what separable_block_eval launches (tap table, bf16 weight, the kernel), with the form named
                return N.sepblock_fwd(xh, N.dwconv_taps(ops[1]), SB._bn_operands(ops[2]), N.pwconv_weight(ops[3]),
                                      SB._bn_operands(ops[4]), s, form=form)

            # the form 'auto' would run comes first; where that is the stream form, the resident form is timed as well
            forms = ["stream", "resident"] if N.sepblock_form(ci, co) == "stream" else ["resident"]
            fused = fused_as(forms[0])
            assert torch.equal(fused, SB.separable_block_eval(*ops, backend="native"))
            chain = layers("native").permute(0, 2, 3, 1)
            differ = float((fused.float() - chain.float()).abs().max())
            res = rounds([lambda f=f: fused_as(f) for f in forms] + [lambda: layers("native"), lambda: layers("torch")])
            nbytes = 2 * (xh.numel() + fused.numel())
            P, tw, kc, R, lds = N.sepblock_geometry(ci)
            lines.append("block {} ({} block{}): {} x {} x {} -> {} x {} x {}, stride {}; resident form: tile 8 x {}, "
                         "weight stage {} k, {:.1f} KB LDS; max |fused ({}) - native layers| {:.3f}".format(
                             ", ".join(str(b + 1) for b in blocks), len(blocks), "s" if len(blocks) > 1 else "", H, W, ci,
                             fused.shape[1], fused.shape[2], co, s, tw, kc, lds / 1024, forms[0], differ))
            for name, (med, lo, hi) in zip(["fused " + f for f in forms] + ["native layers", "torch layers"], res):
                lines.append("  {:<14} {:9.1f} us ({:9.1f} .. {:9.1f})  {:5.2f} TB/s".format(name, med, lo, hi,
                                                                                           nbytes / med * 1e-6))
            if len(forms) == 2:
                lines.append("  stream against resident: {:5.2f}x".format(res[1][0] / res[0][0]))
                res = [res[0]] + res[2:]
            best = min(res[1:], key=lambda r: r[0])
            spread = max(res[0][2] - res[0][1], best[2] - best[1])
            verdict = "LOSES" if res[0][0] > best[0] + spread else "wins" if res[0][0] + spread < best[0] else "level"
            if verdict == "LOSES":
                losers.append((ci, co, s))
            lines.append("  fused against the better of the two: {:5.2f}x ({})".format(best[0] / res[0][0], verdict))
            del xh, x, ops, fused, chain
        lines.append("forms that lose beyond the spread (Ci, Co, stride): {}".format(losers or "none"))

        img = torch.randn(B, 800, 1333, 3, device=dev, generator=g).bfloat16()

        committed = N.SEP_AUTO_EXCLUDED

        def forward(block_backend, layer_backend, excluded=None):
            set_layers(net, layer_backend)
            net.block_backend = block_backend
            N.SEP_AUTO_EXCLUDED = committed if excluded is None else frozenset(excluded)
            try:
                return net(img)
            finally:
                N.SEP_AUTO_EXCLUDED = committed

        # 'auto' three ways: with the committed constant, with what this run found losing, and with every stream form
        # left to the layers, which is the forward before sepblock_stream.hip (blocks 1 to 6 fused, 7 to 13 as layers)
        before = [(ci, co, s) for _, (_, _, ci, co, s) in block_forms(800, 1333) if N.sepblock_form(ci, co) == "stream"]
        res = rounds([lambda: forward("native", "native"), lambda: forward("auto", "native"),
                      lambda: forward("auto", "native", losers), lambda: forward("auto", "native", before),
                      lambda: forward("torch", "native"), lambda: forward("torch", "torch")], calls=3)
        taken = []
        for excluded in (None, losers, before):
            forward("auto", "native", excluded)
            taken.append(" ".join(net.block_taken))
        lines.append("MobileNet(1.0).eval() forward, batch {} of 800 x 1333 ({} rounds x 3 calls); under block_backend = "
                     "'auto' the blocks run as: {}".format(B, ROUNDS, taken[0]))
        lines.append("  with this run's losing forms excluded: {}".format(taken[1]))
        lines.append("  with the stream forms excluded:        {}".format(taken[2]))
        names = ("block_backend 'native' over native layers", "block_backend 'auto' over native layers",
                 "'auto', this run's losing forms excluded", "'auto', stream forms excluded (as before)", "native layers",
                 "torch layers")
        for name, (med, lo, hi) in zip(names, res):
            lines.append("  {:<42} {:9.1f} us ({:9.1f} .. {:9.1f})".format(name, med, lo, hi))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
