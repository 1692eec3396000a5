#!/usr/bin/env python
"""Evaluation throughput, per-image path against the batched path (eval/batched.py), on one GPU.

Writes a 64-image COCO-layout JPEG fixture of COCO-like sizes (scripts/make_coco_fixture.py --sizes coco) into a
temporary directory and runs ``evaluate_coco`` over it with a ResNet-50 RetinaNet of random weights -- first the
per-image path (``batch_size=0``), then ``batch_size=8`` -- two passes each.  The first pass of a path tunes the
convolutions for its shapes; the second is the steady one.  Random weights never reach the 0.05 score threshold,
so the classification bias is raised until about 300 scores per image pass it, the load a trained model puts on
the detection filter and the host side of the evaluation.

usage: bench_eval.py [--n 64] [--eval-batch-size 8] [--eval-pad-multiple 0] [--eval-workers 4] [--passes 2]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--eval-batch-size", type=int, default=8)
    ap.add_argument("--eval-pad-multiple", type=int, default=0)
    ap.add_argument("--eval-workers", type=int, default=4)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()

    import math
    import torch
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.coco import CocoGenerator
    from batchai_retinanet_horovod_coco_amd.eval.coco_eval import evaluate_coco
    from batchai_retinanet_horovod_coco_amd.models.calibrate import calibrate_from_synthetic
    from batchai_retinanet_horovod_coco_amd.ops import native

    assert torch.cuda.is_available(), "bench_eval.py needs a GPU"
    native.load(required=True)
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_coco_fixture.py"), tmp, "--n", str(a.n),
                        "--set", "val2017", "--sizes", "coco", "--workers", "8"], check=True)
        gen = CocoGenerator(tmp, "val2017", shuffle_groups=False)
        torch.manual_seed(0)
        model = models.backbone("resnet50").retinanet(gen.num_classes())
        calibrate_from_synthetic(model, torch.device("cpu"), batch=1, height=256, width=320)
        model = model.to(dev).eval()
        pred = models.retinanet_bbox(model)
        pred.compute_dtype = torch.bfloat16
        # raise the classification bias so that ~300 scores of the first image pass the 0.05 threshold
        image, _ = gen.resize_image(gen.preprocess_image(gen.load_image(0)))
        with torch.no_grad():
            logits = model(torch.from_numpy(image[None]).to(dev).to(torch.bfloat16))["classification"].float().flatten()
            kth = torch.topk(logits, 300).values[-1].item()
            model.classification_submodel.final.bias.add_(math.log(0.05 / 0.95) - kth)
        steady = {}
        for name, kw in (("per-image", {}),
                         ("batched", dict(batch_size=a.eval_batch_size, pad_multiple=a.eval_pad_multiple,
                                          workers=a.eval_workers))):
            for p in range(a.passes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stats = evaluate_coco(gen, pred, results_path=os.path.join(tmp, name + "_bbox_results.json"),
                                      verbose=False, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ndet = 0
                if stats is not None:
                    with open(os.path.join(tmp, name + "_bbox_results.json")) as f:
                        ndet = f.read().count('"image_id"')
                steady[name] = gen.size() / dt
                print("{:9s} pass {}: {:7.2f} s  {:7.2f} images/s  {} detections  AP {:.4f}".format(
                    name, p + 1, dt, gen.size() / dt, ndet, float(stats[0]) if stats is not None else float("nan")),
                    flush=True)
        print("steady images/s: per-image {:.2f}  batched (batch {}, pad {}, {} workers) {:.2f}  ratio {:.2f}x".format(
            steady["per-image"], a.eval_batch_size, a.eval_pad_multiple, a.eval_workers, steady["batched"],
            steady["batched"] / steady["per-image"]))


if __name__ == "__main__":
    main()
