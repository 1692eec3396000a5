"""Device-side batch assembly for real data (HIP normalise + affine warp + bilinear resize + pad).

The reference does all of this on the CPU per image (keras-retinanet ``preprocess_group_entry``:
caffe preprocess -> ``apply_transform`` (cv2.warpAffine) -> ``resize_image`` (cv2.resize) ->
``compute_inputs`` zero padding; SURVEY §2.6 K22, reached from ``/root/reference/train.py:179-193``)
and ships 12.8 MB of float32 per 800x1333 image host->device.  Here the host only decodes the
JPEG and draws the random transform; the uint8 image (4x smaller) goes to the GPU and
``csrc/kernels/image.hip`` does the rest directly into the padded NHWC batch.  Box arithmetic
(transform_aabb, scale) stays on the host, exactly as in the CPU path, so annotations are
bit-identical between the two paths.
"""
from __future__ import annotations

import threading
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ..utils import cpu_native
from .image import CAFFE_MEAN_BGR, compute_resize_scale


# Training batches on a CUDA device: True builds the whole batch with one host->device copy and one launch of
# batch_warp_resize_norm_kernel (bit-identical to the per-image route in caffe mode, tests/test_train_batch_gpu.py);
# False keeps the per-image route (one copy, warp_norm_kernel and resize_kernel per image into a zero-filled batch).
# Read at every batch by DevicePreprocessor.__call__ and ProcessEnqueuer._assemble, so scripts/bench_switch.py and
# scripts/bench_train_batch.py can flip it inside one process.
TRAIN_FUSED = True
# one-launch route of DevicePreprocessor.__call__: start the host->device copy of the packed images every this many
# bytes (an 800x1333 image is 3.2 MB), so a large batch's transfer overlaps the host packing the rest; a batch
# smaller than this goes in one copy
STAGE_CHUNK_BYTES = 4 << 20


def transform_codes(params):
    """(interp, border, cval) of the generator's ``TransformParameters`` as the kernels take them."""
    if params is None:
        return 1, 1, 0.0
    return cpu_native.INTERP[params.interpolation], cpu_native.BORDER[params.fill_mode], float(params.cval)


def normalization(mode: str = "caffe"):
    """(scale, mean) such that ``x*scale - mean`` == ``preprocess_image(x, mode)``."""
    if mode == "caffe":
        return 1.0, CAFFE_MEAN_BGR
    if mode == "tf":
        return 1.0 / 127.5, (1.0, 1.0, 1.0)
    return 1.0, (0.0, 0.0, 0.0)


class DevicePreprocessor:
    """Builds the zero-padded (B, Hmax, Wmax, 3) batch on ``device`` from uint8 BGR images."""

    def __init__(self, device: torch.device, min_side: int = 800, max_side: int = 1333, mode: str = "caffe",
                 dtype: torch.dtype = torch.float32, pad_multiple: int = 0):
        self.device = torch.device(device)
        self.pad_multiple = int(pad_multiple or 0)
        self.min_side, self.max_side = min_side, max_side
        self.scale, self.mean = normalization(mode)
        self.dtype = dtype
        self._stage_lock = threading.Lock()     # loader threads build training batches concurrently

    def output_size(self, hw: Sequence[int]):
        s = compute_resize_scale(hw, min_side=self.min_side, max_side=self.max_side)
        return (int(round(hw[0] * s)), int(round(hw[1] * s))), s

    def __call__(self, images: List[np.ndarray], matrices: List[Optional[np.ndarray]], batch_size: int,
                 params=None) -> torch.Tensor:
        """The training batch of ``images`` (uint8 BGR HWC), image i warped by ``matrices[i]`` (``None``: no warp).
        On a CUDA device with ``TRAIN_FUSED``: one staged copy and one launch (per 32 slots) that writes every value
        of the batch; otherwise :meth:`per_image`."""
        if not (TRAIN_FUSED and self.device.type == "cuda"):
            return self.per_image(images, matrices, batch_size, params)
        from ..ops import native
        from .generator import pad_shape
        sizes = [self.output_size(im.shape[:2])[0] for im in images]
        Hm, Wm = pad_shape((max(s[0] for s in sizes), max(s[1] for s in sizes)), self.pad_multiple)
        interp, border, cval = transform_codes(params)
        staging, offsets = self._stage(images, chunk_bytes=STAGE_CHUNK_BYTES)
        table = [(off, im.shape[0], im.shape[1], oh, ow) for off, im, (oh, ow) in zip(offsets, images, sizes)]
        batch = torch.empty((batch_size, Hm, Wm, 3), dtype=self.dtype, device=self.device)
        native.image_batch_warp_resize_normalize(staging, table, list(matrices), batch, len(images), interp, border,
                                                 cval, self.scale, self.mean)
        return batch

    def per_image(self, images: List[np.ndarray], matrices: List[Optional[np.ndarray]], batch_size: int,
                  params=None) -> torch.Tensor:
        """The per-image route: one copy, warp_norm_kernel into an fp32 image at source size and resize_kernel into
        the zero-filled batch, for each image."""
        from ..ops import native
        sizes = [self.output_size(im.shape[:2])[0] for im in images]
        from .generator import pad_shape
        Hm, Wm = pad_shape((max(s[0] for s in sizes), max(s[1] for s in sizes)), self.pad_multiple)
        batch = torch.zeros((batch_size, Hm, Wm, 3), dtype=self.dtype, device=self.device)
        interp, border, cval = transform_codes(params)
        for i, (im, M, (oh, ow)) in enumerate(zip(images, matrices, sizes)):
            host = torch.from_numpy(np.ascontiguousarray(im, dtype=np.uint8))
            if self.device.type == "cuda":
                host = host.pin_memory()
            src = host.to(self.device, non_blocking=True)
            f = native.image_warp_normalize(src, M, None, interp, border, cval, self.scale, self.mean)
            native.image_resize_into(f, batch, i, (oh, ow))
        return batch

    # ------------------------------------------------------------------ staging (evaluation and one-launch training batches)
    def _stage(self, images: List[np.ndarray], chunk_bytes: int = 0):
        """Pack the uint8 images into one of two pinned host buffers and start ONE async copy to the device.
        The buffers alternate; the event recorded after a buffer's copy is waited for before that buffer is
        written again, so a copy that may still be in flight never reads a half-refilled buffer.

        ``chunk_bytes`` > 0 (training batches): the copy of what is packed so far is started whenever that many
        bytes are waiting, so the transfer of a large batch runs while the host still packs the rest of it."""
        with self._stage_lock:
            return self._stage_locked(images, chunk_bytes)

    def _stage_locked(self, images: List[np.ndarray], chunk_bytes: int = 0):
        st = getattr(self, "_staging", None)
        if st is None:
            st = self._staging = {"next": 0, "host": [None, None], "event": [None, None]}
        offsets, total = [], 0
        for im in images:
            offsets.append(total)
            total += im.shape[0] * im.shape[1] * 3
        k = st["next"]
        st["next"] = k ^ 1
        if st["event"][k] is not None:
            st["event"][k].synchronize()
        cuda = self.device.type == "cuda"
        host = st["host"][k]
        if host is None or host.numel() < total:
            host = st["host"][k] = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=cuda)
        view = host.numpy()
        dev = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        sent = 0
        for im, off in zip(images, offsets):
            n = im.shape[0] * im.shape[1] * 3
            view[off:off + n] = np.ascontiguousarray(im, dtype=np.uint8).reshape(-1)
            if chunk_bytes > 0 and off + n - sent >= chunk_bytes and off + n < total:
                dev[sent:off + n].copy_(host[sent:off + n], non_blocking=True)
                sent = off + n
        dev[sent:total].copy_(host[sent:total], non_blocking=True)
        if cuda:
            if st["event"][k] is None:
                st["event"][k] = torch.cuda.Event()
            st["event"][k].record()
        return dev, offsets

    # ------------------------------------------------------------------ evaluation batches
    def build_eval_batch(self, images: List[np.ndarray], batch_size: int):
        """The evaluation batch of ``images`` (uint8 BGR HWC), built by one kernel launch per 32 slots.

        Returns ``(batch, sizes, scales)``: ``batch`` is ``(batch_size, Hm, Wm, 3)`` with image i normalised and
        resized (``resize_image`` sizes) at the top-left of slot i and zeros elsewhere, ``(Hm, Wm)`` the largest
        resized size padded to ``pad_multiple``; ``sizes[i]`` is image i's resized ``(oh, ow)`` and ``scales[i]`` its
        resize scale.  The kernel writes every value of the batch, so nothing is zero-filled first and no
        full-size fp32 image is materialised."""
        from ..ops import native
        from .generator import pad_shape
        if not 1 <= len(images) <= batch_size:
            raise ValueError("build_eval_batch: {} images for {} slots".format(len(images), batch_size))
        sizes, scales = [], []
        for im in images:
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("build_eval_batch wants HWC images with 3 channels, got {}".format(im.shape))
            (oh, ow), s = self.output_size(im.shape[:2])
            sizes.append((oh, ow))
            scales.append(s)
        Hm, Wm = pad_shape((max(s[0] for s in sizes), max(s[1] for s in sizes)), self.pad_multiple)
        staging, offsets = self._stage(images)
        table = [(off, im.shape[0], im.shape[1], oh, ow) for off, im, (oh, ow) in zip(offsets, images, sizes)]
        batch = torch.empty((batch_size, Hm, Wm, 3), dtype=self.dtype, device=self.device)
        native.image_batch_resize_normalize(staging, table, batch, len(images), self.scale, self.mean)
        return batch, sizes, scales


def compute_input_output_device(gen, group) -> Dict[str, torch.Tensor]:
    """``Generator.compute_input_output`` with the image work on the device (see module doc)."""
    from .transform import adjust_transform_for_image, transform_aabb
    image_group = gen.load_image_group(group)
    annotations_group = gen.load_annotations_group(group)
    image_group, annotations_group = gen.filter_annotations(image_group, annotations_group, group)
    pre: DevicePreprocessor = gen.device_preprocessor
    matrices, sized_shapes = [], []
    for i, (image, ann) in enumerate(zip(image_group, annotations_group)):
        M = None
        ann = ann.copy()
        if gen.transform_generator is not None:
            with gen._transform_lock:
                raw = next(gen.transform_generator)
            M = adjust_transform_for_image(raw, image, gen.transform_parameters.relative_translation)
            for j in range(ann.shape[0]):
                ann[j, :4] = transform_aabb(M, ann[j, :4])
        (oh, ow), s = pre.output_size(image.shape[:2])
        ann[:, :4] *= s
        annotations_group[i] = ann
        matrices.append(M)
        sized_shapes.append((oh, ow))
    images = pre(image_group, matrices, gen.batch_size, gen.transform_parameters)
    B = gen.batch_size
    G = max(1, max(a.shape[0] for a in annotations_group))
    gt = np.full((B, G, 5), -1.0, dtype=np.float32)
    cnt = np.zeros((B,), dtype=np.int32)
    hw = np.zeros((B, 2), dtype=np.int32)
    for i, ann in enumerate(annotations_group):
        gt[i, :ann.shape[0]] = ann
        cnt[i] = ann.shape[0]
        hw[i] = sized_shapes[i]
    for i in range(len(image_group), B):
        hw[i] = images.shape[1:3]
    return {"images": images, "gt": torch.from_numpy(gt), "gt_count": torch.from_numpy(cnt),
            "image_hw": torch.from_numpy(hw)}
