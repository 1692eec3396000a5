"""CPU side of the one-launch training batch: the loader's copy / table plan on hand-made metas, and the routes a CPU
device takes (unchanged by the TRAIN_FUSED switch) against the host pipeline's own functions."""
import numpy as np
import pytest
import torch


def _meta(shape, off, M=None, out_hw=(8, 8), inline=None):
    return (shape, off, M, out_hw, np.zeros((1, 5), dtype=np.float32), inline)


def test_plan_offsets_are_relative_to_the_copied_range():
    from batchai_retinanet_horovod_coco_amd.data.process_loader import plan_train_batch
    M = np.arange(9, dtype=np.float64).reshape(3, 3)
    metas = [_meta((4, 5, 3), 512, M, (8, 10)), _meta((3, 3, 3), 768, None, (6, 6)), _meta((2, 7, 3), 1024, M, (4, 14))]
    lo, span, total, table, mats, inl = plan_train_batch(metas)
    assert (lo, span, total) == (512, 1024 + 2 * 7 * 3 - 512, 1024 + 42 - 512) and inl == []
    assert table == [(0, 4, 5, 8, 10), (256, 3, 3, 6, 6), (512, 2, 7, 4, 14)]
    assert mats[0] is M and mats[1] is None and mats[2] is M
    # the order in the arena need not be the order in the batch
    lo, span, total, table, _, _ = plan_train_batch([metas[2], metas[0]])
    assert (lo, span, total) == (512, 554, 554) and [r[0] for r in table] == [512, 0]


def test_plan_appends_inline_images_after_the_arena_range():
    from batchai_retinanet_horovod_coco_amd.data.process_loader import plan_train_batch
    big = np.zeros((10, 10, 3), dtype=np.uint8)
    metas = [_meta((4, 5, 3), 0), _meta((10, 10, 3), -1, None, (8, 8), big), _meta((2, 2, 3), 256),
             _meta((10, 10, 3), -1, np.eye(3), (8, 8), big)]
    lo, span, total, table, mats, inl = plan_train_batch(metas)
    assert (lo, span) == (0, 256 + 12) and total == span + 2 * 300
    assert [r[0] for r in table] == [0, span, 256, span + 300]
    assert inl == [(span, 1), (span + 300, 3)]
    assert mats[1] is None and mats[3] is not None
    # every image inline: nothing is copied from the arena
    lo, span, total, table, _, inl = plan_train_batch([metas[1], metas[3]])
    assert (lo, span, total) == (0, 0, 600) and [r[0] for r in table] == [0, 300] and inl == [(0, 0), (300, 1)]
    with pytest.raises(ValueError):
        plan_train_batch([_meta((4, 5), 0)])


def test_plan_rows_pass_the_table_checks():
    """Each planned image lies inside the staging buffer and the images do not overlap."""
    from batchai_retinanet_horovod_coco_amd.data.process_loader import plan_train_batch
    metas = [_meta((7, 9, 3), 256), _meta((5, 5, 3), -1, None, (8, 8), np.zeros((5, 5, 3), np.uint8)),
             _meta((1, 1, 3), 0)]
    _, _, total, table, _, _ = plan_train_batch(metas)
    spans = sorted((r[0], r[0] + r[1] * r[2] * 3) for r in table)
    assert spans[0][0] >= 0 and spans[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def _host_batch(images, matrices, pre, params, batch_size):
    """preprocess_image -> apply_transform -> resize_image -> zero pad, as Generator.preprocess_group_entry."""
    from batchai_retinanet_horovod_coco_amd.data.generator import pad_shape
    from batchai_retinanet_horovod_coco_amd.data.image import apply_transform, preprocess_image, resize_image
    outs = []
    for im, M in zip(images, matrices):
        f = preprocess_image(im)
        if M is not None:
            f = apply_transform(M, f, params)
        outs.append(resize_image(f, min_side=pre.min_side, max_side=pre.max_side)[0])
    Hm, Wm = pad_shape((max(o.shape[0] for o in outs), max(o.shape[1] for o in outs)), pre.pad_multiple)
    want = np.zeros((batch_size, Hm, Wm, 3), dtype=np.float32)
    for i, o in enumerate(outs):
        want[i, :o.shape[0], :o.shape[1]] = o
    return want


@pytest.mark.parametrize("fused", [True, False])
def test_cpu_device_keeps_the_per_image_route(monkeypatch, fused):
    """On a CPU device DevicePreprocessor.__call__ is the per-image route whatever the switch says: it calls the two
    per-image entry points (stood in for here by the host functions they mirror, a CPU tensor cannot reach a HIP
    kernel) and never the one-launch entry or the staging buffers, and the batch is the host pipeline's."""
    from batchai_retinanet_horovod_coco_amd.data import device_preprocess as dp
    from batchai_retinanet_horovod_coco_amd.data.image import TransformParameters, apply_transform, preprocess_image
    from batchai_retinanet_horovod_coco_amd.data.transform import adjust_transform_for_image, scaling
    from batchai_retinanet_horovod_coco_amd.ops import native
    from batchai_retinanet_horovod_coco_amd.utils import cpu_native
    params = TransformParameters()
    calls = {"warp": 0, "resize": 0}

    def warp(src, matrix=None, out_hw=None, interp=1, border=1, cval=0.0, scale=1.0, mean=(0.0, 0.0, 0.0)):
        calls["warp"] += 1
        assert (interp, border, cval) == dp.transform_codes(params) and (scale, tuple(mean)) == dp.normalization("caffe")
        f = preprocess_image(src.numpy())
        return torch.from_numpy(f if matrix is None else apply_transform(matrix, f, params))

    def resize(src, batch, index, out_hw):
        calls["resize"] += 1
        batch[index, :out_hw[0], :out_hw[1]] = torch.from_numpy(cpu_native.resize_bilinear(src.numpy(), *out_hw))

    def never(*a, **k):
        raise AssertionError("the one-launch route ran on a CPU device")

    monkeypatch.setattr(native, "image_warp_normalize", warp)
    monkeypatch.setattr(native, "image_resize_into", resize)
    monkeypatch.setattr(native, "image_batch_warp_resize_normalize", never)
    monkeypatch.setattr(dp.DevicePreprocessor, "_stage", never)
    monkeypatch.setattr(dp, "TRAIN_FUSED", fused)
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in [(40, 50), (50, 40), (33, 47)]]
    mats = [None, adjust_transform_for_image(scaling((-1, 1)), images[1], True), None]
    pre = dp.DevicePreprocessor(torch.device("cpu"), 64, 96, pad_multiple=32)
    got = pre(images, mats, 4, params)
    assert calls == {"warp": 3, "resize": 3}
    want = _host_batch(images, mats, pre, params, 4)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("fused", [True, False])
def test_assemble_host_matches_host_functions(monkeypatch, fused):
    """The loader's CPU assembly (arena and inline images) against preprocess_image / apply_transform / resize_image,
    with the switch on and off."""
    from batchai_retinanet_horovod_coco_amd.data import device_preprocess as dp
    from batchai_retinanet_horovod_coco_amd.data.image import TransformParameters
    from batchai_retinanet_horovod_coco_amd.data.synthetic import SyntheticGenerator
    from batchai_retinanet_horovod_coco_amd.data.process_loader import ProcessEnqueuer
    from batchai_retinanet_horovod_coco_amd.data.transform import adjust_transform_for_image, scaling
    import queue
    monkeypatch.setattr(dp, "TRAIN_FUSED", fused)
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in [(40, 50), (44, 50), (36, 50)]]
    mats = [adjust_transform_for_image(scaling((-1, 1)), images[0], True), None, None]
    params = TransformParameters()
    pre = dp.DevicePreprocessor(torch.device("cpu"), 64, 96)
    gen = SyntheticGenerator(num_images=4, height=40, width=50, batch_size=4, image_min_side=64, image_max_side=96,
                             transform_parameters=params, cache_bytes=0)
    gen.device_preprocessor = pre
    arena = torch.zeros((2, 16384), dtype=torch.uint8)
    metas, off = [], 256
    for k, (im, M) in enumerate(zip(images, mats)):
        oh, ow = pre.output_size(im.shape[:2])[0]
        ann = np.array([[1, 2, 30, 20, k]], dtype=np.float32)
        if k == 2:
            metas.append((im.shape, -1, M, (oh, ow), ann, im))
            continue
        arena[1, off:off + im.size] = torch.from_numpy(im.reshape(-1))
        metas.append((im.shape, off, M, (oh, ow), ann, None))
        off += (im.size + 255) // 256 * 256
    enq = object.__new__(ProcessEnqueuer)        # the assembly alone: no workers, no shared memory
    enq.__dict__.update(gen=gen, arena=arena, free=queue.Queue(), stats={"batches": 0, "images": 0},
                        device=torch.device("cpu"))
    out, ev = enq._assemble(1, metas)
    assert ev is None and enq.free.get_nowait() == 1 and enq.stats == {"batches": 1, "images": 3}
    want = _host_batch(images, mats, pre, params, 4)
    assert np.array_equal(out["images"].numpy(), want)
    assert out["gt_count"].tolist() == [1, 1, 1, 0] and out["gt"][2, 0, 4] == 2
    assert out["image_hw"].tolist()[:3] == [list(m[3]) for m in metas]
