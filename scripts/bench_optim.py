"""Fused optimizer steps on ResNet-50 RetinaNet's flat buffers (the real model, bf16 compute copies on), Adam and
the SGD forms alternating in one process:  python scripts/bench_optim.py [--reps 15] [--calls 20]
Each repetition times ``calls`` back-to-back steps of every form with device events; prints microseconds per step
(median and the spread over the repetitions) and the HBM rate of the bytes the form moves per element
(Adam: p, g, m, v read, p, m, v and the bf16 copy written = 30 B; SGD: p, g, v read, p, v and the copy written = 22 B;
the weight EMA fused into the launch adds one fp32 read and write = 8 B, a separate ``lerp_`` pass over p and the average 12 B,
``mul_`` then ``add_`` 8 + 12 B).
The ``adam, then ...`` rows are what a user's own EMA after the step costs: the plain fused step followed by
``ema.lerp_(p, 1 - d)`` or by ``ema.mul_(d).add_(p, alpha=1 - d)`` with a host-computed ``d``."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchai_retinanet_horovod_coco_amd import models  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native as N  # noqa: E402
from batchai_retinanet_horovod_coco_amd.train.engine import Trainer  # noqa: E402
from batchai_retinanet_horovod_coco_amd.train.optimizer import KerasAdam, KerasSGD  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py times HIP kernels: it needs a GPU")
    N.load(required=True)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = Trainer(models.backbone("resnet50").retinanet(80), compute_dtype=torch.bfloat16, device=dev)
    flat, plan = tr.flat, tr.adam_plan()
    assert tr.compute_weights is not None and plan.copy is not None
    flat.grad.normal_()
    scale = torch.full((), 1e-3, device=dev)
    lr = 1e-6       # the weights stay finite however many steps are timed
    D = 0.9998
    own = flat.data.clone()         # the average of the two-launch rows

    def lerp(opt):
        own.lerp_(flat.data, 1.0 - opt.ema_decay_at(opt.iterations))

    def mul_add(opt):
        d = opt.ema_decay_at(opt.iterations)
        own.mul_(d).add_(flat.data, alpha=1.0 - d)

    post = {"adam, then lerp_": lerp, "adam, then mul_/add_": mul_add}
    two = KerasAdam(flat, lr=lr)
    two.ema_decay = D               # only for ema_decay_at: no buffer, the plain fused step
    forms = [
        ("adam", 30, KerasAdam(flat, lr=lr)),
        ("sgd plain", 22, KerasSGD(flat, lr=lr)),
        ("sgd momentum", 22, KerasSGD(flat, lr=lr, momentum=0.9)),
        ("sgd nesterov", 22, KerasSGD(flat, lr=lr, momentum=0.9, nesterov=True)),
        ("sgd momentum+decay", 22, KerasSGD(flat, lr=lr, momentum=0.9, weight_decay=1e-4)),
        ("adam+ema", 38, KerasAdam(flat, lr=lr, ema_decay=D)),
        ("sgd momentum+ema", 30, KerasSGD(flat, lr=lr, momentum=0.9, ema_decay=D)),
        ("adam, then lerp_", 42, two),
        ("adam, then mul_/add_", 50, two),
    ]
    its = {name: 0 for name, _, _ in forms}

    def run(name, opt, n):
        # every form keeps its own step count; the plan's device counter is shared, so it is put right first
        opt.iterations = its[name]
        after = post.get(name)
        for _ in range(n):
            opt.apply(scale)
            if after is not None:
                after(opt)
        its[name] = opt.iterations

    for name, _, opt in forms:
        run(name, opt, 3)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in forms}
    for _ in range(args.reps):
        for name, _, opt in forms:
            plan.sync_iter(its[name])
            plan.set_lr(opt.base_lr(its[name] + 1))
            if hasattr(opt, "momentum"):
                plan.set_momentum(opt.momentum)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, opt, args.calls)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / args.calls)
    assert bool(torch.isfinite(flat.data).all())
    n = sum(s.numel for s in flat.segments)
    print("R50 RetinaNet(80): {:,} parameters in {} segments, {} chunks; {} repetitions x {} steps per form"
          .format(n, len(flat.segments), plan.nchunks, args.reps, args.calls))
    print("{:<22} {:>10} {:>10} {:>10} {:>8} {:>9}".format("form", "median us", "min us", "max us", "B/elem", "TB/s"))
    for name, nbytes, _ in forms:
        t = sorted(times[name])
        med = t[len(t) // 2]
        print("{:<22} {:>10.1f} {:>10.1f} {:>10.1f} {:>8} {:>9.2f}".format(name, med, t[0], t[-1], nbytes,
                                                                          n * nbytes / (med * 1e-6) / 1e12))
    adam = sorted(times["adam"])
    spread = adam[-1] - adam[0]
    for name, _, _ in forms[1:5]:
        t = sorted(times[name])
        d = t[len(t) // 2] - adam[len(adam) // 2]
        print("{:<22} median {:+.1f} us against adam (adam's own spread over repetitions: {:.1f} us){}".format(
            name, d, spread, "  SLOWER THAN ADAM BY MORE THAN THE SPREAD" if d > spread else ""))
    med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    for name, nbytes in (("adam, then lerp_", 42), ("adam, then mul_/add_", 50)):
        d = med["adam+ema"] - med[name]
        print("adam+ema               median {:+.1f} us against '{}' ({:.2f} x; expected from the bytes {:.2f} x){}"
              .format(d, name, med["adam+ema"] / med[name], 38 / nbytes,
                      "" if d < -spread else "  NOT FASTER BEYOND ADAM'S SPREAD"))
    print("adam+ema               median {:+.1f} us against adam; sgd momentum+ema {:+.1f} us against sgd momentum"
          .format(med["adam+ema"] - med["adam"], med["sgd momentum+ema"] - med["sgd momentum"]))


if __name__ == "__main__":
    main()
