"""Batched, rank-sharded detection collection for the evaluation callbacks (``--eval-batch-size``).

The per-image path (``coco_eval.predict_image``) preprocesses on the host, runs batch-1 forwards on rank 0 only
and copies three tensors back per image.  Here every rank takes a share of the images: they are grouped by the
shape of their resized tensor (:func:`plan_batches`), decoded by a thread pool two batches ahead, turned into a
batch by one kernel launch (``DevicePreprocessor.build_eval_batch``), run through the prediction model once per
batch, finished on the device (``native.finish_detections``: clip to the image's own size, undo the resize scale,
count the rows above the threshold) and brought back with one copy per batch.  :func:`gather_detections` merges
the ranks' shares, so the evaluation itself (rank 0) sees exactly what the per-image loop would have produced.

With ``pad_multiple = 0`` a batch holds only images whose resized shape is identical, so each image gets exactly
the tensor ``predict_image`` gives it.  A non-zero multiple pads to shape classes instead (see the README for the
deviation: anchors in the padding, and the clip to the image's own size applied after NMS instead of before).
"""
from __future__ import annotations

from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from ..data.generator import pad_shape
from ..data.image import compute_resize_scale, preprocess_image, read_image_size
from ..parallel import collectives, runtime


def _world() -> Tuple[int, int]:
    """(rank, world size); (0, 1) outside a data-parallel job."""
    if not runtime.is_initialized():
        return 0, 1
    return runtime.rank(), runtime.size()


def resized_hw(hw: Sequence[int], min_side: int, max_side: int) -> Tuple[int, int]:
    """The (oh, ow) ``resize_image`` gives an image of size ``hw``."""
    s = compute_resize_scale(hw, min_side=min_side, max_side=max_side)
    return int(round(hw[0] * s)), int(round(hw[1] * s))


def plan_batches(hw_list: Sequence[Sequence[int]], batch_size: int, min_side: int, max_side: int,
                 pad_multiple: int = 0, world: int = 1) -> List[List[List[int]]]:
    """Which images every rank evaluates together: ``plan[rank]`` is that rank's list of batches (image indices).

    Pure and deterministic -- every rank computes the whole plan.  An image's key is its resized shape padded to
    ``pad_multiple`` (0: the exact resized shape); indices are sorted by (key, index), every run of one key is cut
    into batches of at most ``batch_size``, and batch j belongs to rank ``j % world``."""
    if batch_size < 1 or world < 1:
        raise ValueError("plan_batches needs batch_size >= 1 and world >= 1")
    keys = [tuple(pad_shape(resized_hw(hw, min_side, max_side), pad_multiple)) for hw in hw_list]
    order = sorted(range(len(keys)), key=lambda i: (keys[i], i))
    batches: List[List[int]] = []
    for i in order:
        if batches and len(batches[-1]) < batch_size and keys[batches[-1][0]] == keys[i]:
            batches[-1].append(i)
        else:
            batches.append([i])
    return [batches[r::world] for r in range(world)]


def image_hw(generator, i: int) -> Tuple[int, int]:
    """Original (h, w) of image ``i`` without decoding it where the dataset allows: COCO metadata, else the image
    header, else a decode.  It only groups images -- a batch's real shape comes from the decoded images."""
    coco = getattr(generator, "coco", None)
    if coco is not None:
        info = coco.loadImgs(generator.image_ids[i])[0]
        return int(info["height"]), int(info["width"])
    if hasattr(generator, "image_path"):
        return tuple(read_image_size(generator.image_path(i)))
    return tuple(generator.load_image(i).shape[:2])


def _model_device_dtype(prediction_model):
    try:
        dev = next(prediction_model.model.parameters()).device
    except (AttributeError, StopIteration):
        dev = torch.device("cpu")
    dt = getattr(prediction_model, "compute_dtype", None) or (torch.bfloat16 if dev.type == "cuda" else torch.float32)
    return dev, dt


def _host_batch(generator, images, pad_multiple: int):
    """CPU batch: the per-image preprocessing of ``predict_image``, zero padded to a common shape."""
    done, sizes, scales = [], [], []
    for im in images:
        x, s = generator.resize_image(generator.preprocess_image(im))
        done.append(x)
        sizes.append(x.shape[:2])
        scales.append(s)
    Hm, Wm = pad_shape((max(s[0] for s in sizes), max(s[1] for s in sizes)), pad_multiple)
    batch = np.zeros((len(images), Hm, Wm, 3), dtype=np.float32)
    for i, x in enumerate(done):
        batch[i, :x.shape[0], :x.shape[1]] = x
    return torch.from_numpy(batch), sizes, scales


def collect_detections(generator, prediction_model, batch_size: int, pad_multiple: int = 0, workers: int = 4,
                       threshold: float = 0.05) -> Dict[int, Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """Run this rank's batches; ``{image_index: (boxes (n, 4), scores (n), labels (n))}`` with boxes in the
    coordinates of the original image and n the number of leading detections with score >= ``threshold``."""
    from ..data.device_preprocess import DevicePreprocessor
    from ..ops import native
    rank, world = _world()
    hws = [image_hw(generator, i) for i in range(generator.size())]
    mine = plan_batches(hws, batch_size, generator.image_min_side, generator.image_max_side, pad_multiple,
                        world)[rank]
    dev, dt = _model_device_dtype(prediction_model)
    on_gpu = dev.type == "cuda" and native.available() and generator.preprocess_image is preprocess_image
    pre = None
    if on_gpu:
        pre = DevicePreprocessor(dev, generator.image_min_side, generator.image_max_side, "caffe", dt,
                                 pad_multiple=pad_multiple)
    out: Dict[int, Tuple[np.ndarray, np.ndarray, np.ndarray]] = {}
    pool = ThreadPoolExecutor(max_workers=workers) if workers > 0 else None
    todo = iter(mine)
    ahead = deque()

    def submit():
        idx = next(todo, None)
        if idx is not None:
            ahead.append((idx, [pool.submit(generator.load_image, i) for i in idx] if pool else None))

    try:
        submit()
        submit()
        while ahead:
            idx, futures = ahead.popleft()
            submit()                       # the pool now decodes the two batches after this one
            images = [f.result() for f in futures] if futures else [generator.load_image(i) for i in idx]
            if on_gpu:
                batch, sizes, scales = pre.build_eval_batch(images, len(images))
            else:
                batch, sizes, scales = _host_batch(generator, images, pad_multiple)
                batch = batch.to(dev).to(dt)
            boxes, scores, labels = prediction_model(batch)
            table = [(oh, ow, s) for (oh, ow), s in zip(sizes, scales)]
            B, D = int(scores.shape[0]), int(scores.shape[1])
            if boxes.is_cuda and native.available():
                flat = native.finish_detections(boxes.float(), scores.float(), labels.to(torch.int32), table,
                                                threshold, packed=True)
                rows, count = native.unpack_detections(flat, B, D)
            else:
                rows, count = native.finish_detections_host(boxes.float().cpu().numpy(), scores.float().cpu().numpy(),
                                                            labels.cpu().numpy(), table, threshold)
            for b, i in enumerate(idx):
                n = int(count[b])
                out[i] = (rows[b, :n, :4].copy(), rows[b, :n, 4].copy(), rows[b, :n, 5].astype(np.int32))
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)
    return out


def merge_detections(parts: Sequence[dict], size: int = None) -> dict:
    """One dict from every rank's share; an index held twice, or one of ``range(size)`` held by nobody, raises."""
    merged, twice = {}, []
    for part in parts:
        for i, v in part.items():
            if i in merged:
                twice.append(i)
            merged[i] = v
    n = size if size is not None else (max(merged) + 1 if merged else 0)
    missing = [i for i in range(n) if i not in merged]
    extra = [i for i in merged if not 0 <= i < n]
    if twice or missing or extra:
        raise RuntimeError("gather_detections: images evaluated twice {}, missing {}, out of range {}".format(
            sorted(twice)[:8], missing[:8], sorted(extra)[:8]))
    return merged


def gather_detections(local: dict, size: int = None) -> dict:
    """Every rank's detections on every rank.  All ranks see the same gathered shares, so a bad plan (an image
    evaluated twice or by nobody; ``size`` = the dataset's image count) raises on all of them alike."""
    if _world()[1] == 1:
        return local
    return merge_detections(collectives.allgather_object(local), size)
