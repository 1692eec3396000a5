#!/usr/bin/env python
"""Training batch assembly, per-image route against the one-launch route (data.device_preprocess.TRAIN_FUSED), on
one GPU, in one process.

A batch is B seeded uint8 images of one orientation (480x640 or 640x480; the loaders group by aspect ratio), resized
to 800x1067 / 1067x800 into a canvas padded to a multiple of 32.  Two ways in are timed: ``DevicePreprocessor.__call__``
(the thread loader: images in host memory) and ``ProcessEnqueuer._assemble`` (the process loader: images in a slot of
its registered shared-memory arena, on its copy stream, no worker started).  ``flip``: every second image carries the
x-flip the generators draw and the others the identity they draw otherwise; ``affine``: every image carries a general
affine (rotation 0.1, shear 0.05, scale 1.1, translation).

Each timed region is ``--reps`` batches (landscape and portrait in turn), each followed by a synchronize of the
stream it ran on; the routes alternate ``--alternations`` times and every round is printed.  A row counts as a win
only if the slowest one-launch round beats the fastest per-image round.

usage: bench_train_batch.py [--reps 20] [--alternations 3] [--warmup 3] [--batch-sizes 1 16]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(480, 640), (640, 480)]
MIN_SIDE, MAX_SIDE, PAD = 800, 1333, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()

    from batchai_retinanet_horovod_coco_amd.data import process_loader
    assert process_loader.prestart()          # before anything touches the GPU
    import numpy as np
    import torch
    from batchai_retinanet_horovod_coco_amd.data import device_preprocess as dp
    from batchai_retinanet_horovod_coco_amd.data import transform as T
    from batchai_retinanet_horovod_coco_amd.data.image import TransformParameters
    from batchai_retinanet_horovod_coco_amd.data.synthetic import SyntheticGenerator
    from batchai_retinanet_horovod_coco_amd.ops import native

    assert torch.cuda.is_available(), "bench_train_batch.py needs a GPU"
    native.load(required=True)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)

    def matrices(kind, images):
        if kind == "affine":
            m = np.linalg.multi_dot([T.rotation(0.1), T.translation((2.5, -1.25)), T.shear(0.05),
                                     T.scaling((1.1, 1.1))])
            return [T.adjust_transform_for_image(m, im, False) for im in images]
        return [T.adjust_transform_for_image(T.scaling((-1 if i % 2 == 0 else 1, 1)), im, True)
                for i, im in enumerate(images)]

    def sync():
        torch.cuda.current_stream().synchronize()

    def timed(build, batches):
        t0 = time.perf_counter()
        for r in range(a.reps):
            build(batches[r % len(batches)])
        return 1000 * (time.perf_counter() - t0) / a.reps

    def compare(name, build, batches, same):
        """Alternate the routes; ``build(batch)`` ends in a synchronize.  ``same``: the two routes' batches are equal."""
        rounds = {False: [], True: []}
        for fused in (False, True):
            dp.TRAIN_FUSED = fused
            for _ in range(a.warmup):
                for b in batches:
                    build(b)
        for _ in range(a.alternations):
            for fused in (False, True):
                dp.TRAIN_FUSED = fused
                rounds[fused].append(timed(build, batches))
        dp.TRAIN_FUSED = True
        old, new = rounds[False], rounds[True]
        win = max(new) < min(old)
        fmt = lambda v: " ".join("{:7.3f}".format(x) for x in v)       # noqa: E731
        print("{:34s} per-image ms/batch [{}]  one-launch [{}]  median {:7.3f} -> {:7.3f} ({:.2f}x)  spread {:.3f} / "
              "{:.3f}  {}  {}".format(name, fmt(old), fmt(new), float(np.median(old)), float(np.median(new)),
                                      float(np.median(old)) / float(np.median(new)), max(old) - min(old),
                                      max(new) - min(new), "FASTER" if win else "NOT FASTER THAN THE SPREAD",
                                      "bits equal" if same else "BITS DIFFER"), flush=True)

    print("device {}  reps {}  alternations {}  warmup {}".format(torch.cuda.get_device_name(0), a.reps, a.alternations,
                                                                a.warmup), flush=True)
    for B in a.batch_sizes:
        for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            for kind in ("flip", "affine"):
                if kind == "affine" and dtype != torch.bfloat16:
                    continue
                batches = []
                for hw in SIZES:
                    images = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for _ in range(B)]
                    batches.append((images, matrices(kind, images)))
                tag = "B={:<2d} {} {}".format(B, dname, kind)

                # ---- DevicePreprocessor.__call__
                pre = dp.DevicePreprocessor(dev, MIN_SIDE, MAX_SIDE, "caffe", dtype, pad_multiple=PAD)
                params = TransformParameters()

                def call(b):
                    out = pre(b[0], b[1], B, params)
                    sync()
                    return out
                outs = []
                for fused in (False, True):
                    dp.TRAIN_FUSED = fused
                    outs.append([call(b) for b in batches])
                same = all(torch.equal(x, y) for x, y in zip(*outs))
                assert tuple(outs[0][0].shape[1:3]) == (800, 1088) and tuple(outs[0][1].shape[1:3]) == (1088, 800)
                del outs
                compare(tag + " DevicePreprocessor", call, batches, same)

                # ---- ProcessEnqueuer._assemble from its arena (one slot per orientation)
                gen = SyntheticGenerator(num_images=B, height=480, width=640, batch_size=B, image_min_side=MIN_SIDE,
                                         image_max_side=MAX_SIDE, cache_bytes=0, pad_multiple=PAD)
                gen.device_preprocessor = pre
                enq = process_loader.ProcessEnqueuer(gen, workers=1, max_queue_size=2, device=dev)
                try:
                    slots = []
                    for s, (images, mats) in enumerate(batches):
                        metas, off = [], 0
                        for im, M in zip(images, mats):
                            enq.arena[s, off:off + im.size] = torch.from_numpy(im.reshape(-1))
                            metas.append((im.shape, off, M, pre.output_size(im.shape[:2])[0],
                                          np.zeros((1, 5), dtype=np.float32), None))
                            off += (im.size + 255) // 256 * 256
                        slots.append((s, metas))

                    def assemble(sm):
                        out, ev = enq._assemble(sm[0], sm[1])      # waits for its own event on the copy stream
                        enq.free.get_nowait()
                        return out["images"]
                    outs = []
                    for fused in (False, True):
                        dp.TRAIN_FUSED = fused
                        outs.append([assemble(sm) for sm in slots])
                    torch.cuda.synchronize()
                    same = all(torch.equal(x, y) for x, y in zip(*outs))
                    del outs
                    compare(tag + " ProcessEnqueuer (arena {})".format("registered" if enq._registered else "pageable"),
                            assemble, slots, same)
                finally:
                    enq.stop()


if __name__ == "__main__":
    main()
