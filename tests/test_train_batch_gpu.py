"""GPU side of the one-launch training batch: batch_warp_resize_norm_kernel against the per-image route it replaces
(warp_norm_kernel into an fp32 image at source size, then resize_kernel into a zeroed batch), and the two routes of
DevicePreprocessor.__call__ and of the process loader behind the TRAIN_FUSED switch."""
import numpy as np
import pytest
import torch

from eval_batched_common import MAX_SIDE, MIN_SIDE, make_generator, write_fixture

pytestmark = pytest.mark.gpu

CASES = [((5, 7), (8, 11)), ((33, 47), (20, 29)), ((1, 9), (3, 27)), ((16, 16), (16, 16))]
CAFFE = (1.0, (103.939, 116.779, 123.68))
TF = (1.0 / 127.5, (1.0, 1.0, 1.0))
INTERP = {"nearest": 0, "linear": 1}
BORDER = {"constant": 0, "nearest": 1, "reflect": 2, "wrap": 3}
CVAL = 7.5


def _images(cases, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w), _ in cases]


def _flip(im):
    """The x-flip the generators draw (flip_x_chance), as adjust_transform_for_image hands it to the warp."""
    from batchai_retinanet_horovod_coco_amd.data.transform import adjust_transform_for_image, scaling
    return adjust_transform_for_image(scaling((-1, 1)), im, True)


def _affine(im):
    """rotation 0.1 rad, translation (2.5, -1.25) px, shear 0.05, scale 1.1, about the image centre."""
    from batchai_retinanet_horovod_coco_amd.data import transform as T
    m = np.linalg.multi_dot([T.rotation(0.1), T.translation((2.5, -1.25)), T.shear(0.05), T.scaling((1.1, 1.1))])
    return T.adjust_transform_for_image(m, im, False)


def _half_pixel(im):
    from batchai_retinanet_horovod_coco_amd.data.transform import translation
    return translation((0.5, 0.5)).astype(np.float64)


KINDS = [lambda im: None, _flip, _affine, _half_pixel]


def _matrices(images, rot):
    """One matrix per image; ``rot`` rotates the kinds, so over rot = 0..3 every image meets every kind."""
    return [KINDS[(i + rot) % 4](im) for i, im in enumerate(images)]


def _stage(images, dev):
    flat = np.concatenate([im.reshape(-1) for im in images])
    offs = np.cumsum([0] + [im.size for im in images])[:-1]
    return torch.from_numpy(flat).to(dev), [int(o) for o in offs]


def _two_kernel(images, matrices, targets, shape, dtype, norm, dev, interp=1, border=1, cval=0.0):
    """Today's route: warp_norm_kernel at source size, then resize_kernel into a pre-zeroed batch."""
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    ref = torch.zeros(shape, dtype=dtype, device=dev)
    for i, (im, M, hw) in enumerate(zip(images, matrices, targets)):
        f = N.image_warp_normalize(torch.from_numpy(im).to(dev), M, None, interp, border, cval, norm[0], norm[1])
        N.image_resize_into(f, ref, i, hw)
    return ref


def _one_launch(images, matrices, targets, shape, dtype, norm, dev, interp=1, border=1, cval=0.0):
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    staging, offs = _stage(images, dev)
    table = [(o, im.shape[0], im.shape[1], oh, ow) for o, im, (oh, ow) in zip(offs, images, targets)]
    batch = torch.full(shape, float("nan"), dtype=dtype, device=dev)
    N.image_batch_warp_resize_normalize(staging, table, matrices, batch, len(images), interp, border, cval, norm[0],
                                        norm[1])
    return batch


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("slot", [(24, 32), (24, 29)], ids=["24x32", "24x29"])
@pytest.mark.parametrize("border", ["constant", "nearest", "reflect", "wrap"])
@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_train_batch_caffe_bit_identical(cuda, interp, border, slot, dtype):
    """Caffe mode, 6 slots, 4 images, each image under each kind of matrix (none, x-flip, general affine, half-pixel
    translation): bit-identical to the two-kernel route, NaN prefill gone, padding and the two empty slots exactly
    zero.  24x32 has a 16-byte-aligned row pitch (vector stores), 24x29 has not (the scalar tail)."""
    images = _images(CASES)
    targets = [t for _, t in CASES]
    shape = (6,) + slot + (3,)
    kw = dict(interp=INTERP[interp], border=BORDER[border], cval=CVAL)
    for rot in range(4):
        mats = _matrices(images, rot)
        got = _one_launch(images, mats, targets, shape, dtype, CAFFE, cuda, **kw)
        ref = _two_kernel(images, mats, targets, shape, dtype, CAFFE, cuda, **kw)
        assert not torch.isnan(got.float()).any()
        assert torch.equal(got, ref) and torch.equal(_bits(got), _bits(ref))
        assert int(_bits(got)[4:].ne(0).sum()) == 0
        for i, (oh, ow) in enumerate(targets):
            assert int(_bits(got)[i, oh:].ne(0).sum()) == 0 and int(_bits(got)[i, :, ow:].ne(0).sum()) == 0
            assert got[i, :oh, :ow].float().abs().sum() > 0


def test_train_batch_more_than_one_launch(cuda):
    """Two more slots than one launch takes, one fewer image than slots (the last slot empty), every kind of matrix."""
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    slots = N.BATCH_SLOTS + 2
    cases = [((9 + i % 5, 7 + i % 3), (12, 16)) for i in range(slots - 1)]
    images = _images(cases, seed=2)
    targets = [c[1] for c in cases]
    mats = _matrices(images, 1)
    shape = (slots, 12, 16, 3)
    got = _one_launch(images, mats, targets, shape, torch.float32, CAFFE, cuda)
    ref = _two_kernel(images, mats, targets, shape, torch.float32, CAFFE, cuda)
    assert torch.equal(_bits(got), _bits(ref))
    assert int(_bits(got)[slots - 1].ne(0).sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("border", ["constant", "reflect"])
def test_train_batch_tiles_and_register_path(cuda, border, dtype):
    """A block stages the warped source pixels of a tile (8 rows x 128 fp32 / 256 bf16 pixels) in LDS when they fit.
    (37, 150) -> (30, 300) spans four tile rows and two or three tile columns, the last ones partial, under the
    general affine and under the flip; (200, 300) -> (8, 12) names 200 x 300 source pixels from one tile, far more
    than fit, so its taps are evaluated in registers."""
    cases = [((37, 150), (30, 300)), ((200, 300), (8, 12)), ((37, 150), (30, 300))]
    images = _images(cases, seed=4)
    targets = [c[1] for c in cases]
    mats = [_affine(images[0]), _affine(images[1]), _flip(images[2])]
    shape = (3, 32, 304, 3)
    kw = dict(interp=1, border=BORDER[border], cval=CVAL)
    got = _one_launch(images, mats, targets, shape, dtype, CAFFE, cuda, **kw)
    ref = _two_kernel(images, mats, targets, shape, dtype, CAFFE, cuda, **kw)
    assert not torch.isnan(got.float()).any() and torch.equal(_bits(got), _bits(ref))
    for i, (oh, ow) in enumerate(targets):
        assert got[i, :oh, :ow].float().abs().sum() > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_train_batch_production_shape(cuda, dtype):
    """(480, 640) -> (800, 1067) into an 800x1088 slot with the flip matrix: many blocks, the reference job's shape."""
    cases = [((480, 640), (800, 1067))]
    images = _images(cases, seed=1)
    mats = [_flip(images[0])]
    shape = (1, 800, 1088, 3)
    got = _one_launch(images, mats, [cases[0][1]], shape, dtype, CAFFE, cuda)
    ref = _two_kernel(images, mats, [cases[0][1]], shape, dtype, CAFFE, cuda)
    assert torch.equal(_bits(got), _bits(ref))
    assert got[0, :800, :1067].float().abs().sum() > 0


def test_train_batch_tf_mode(cuda):
    """tf mode (x / 127.5 - 1, values in [-1, 1]): only the contraction of ``x*scale - m`` into an FMA may differ
    between the two routes.  The bound of test_batch_builder_tf_mode (4 taps' worth of half-ulp roundings at
    magnitude <= 1, doubled by the two lerps) carried through the second lerp stage: 4 * 2^-24 * 2 * 2 = 9.6e-7.
    Observed maximum on an MI355X: 0.0 (the compiler contracts both routes alike)."""
    images = _images(CASES, seed=3)
    targets = [c[1] for c in CASES]
    shape = (6, 24, 32, 3)
    worst = 0.0
    for rot in range(4):
        mats = _matrices(images, rot)
        got = _one_launch(images, mats, targets, shape, torch.float32, TF, cuda)
        ref = _two_kernel(images, mats, targets, shape, torch.float32, TF, cuda)
        assert float(ref.abs().max()) <= 1.0 + 2.0 ** -22 and not torch.isnan(got).any()
        worst = max(worst, float((got - ref).abs().max()))
    print("tf mode max |diff| = {:.3e}".format(worst))
    assert worst <= 4 * 2.0 ** -24 * 2 * 2


def test_train_batch_rejects_bad_arguments(cuda):
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    staging = torch.zeros(5 * 7 * 3, dtype=torch.uint8, device=cuda)
    batch = torch.empty((2, 8, 8, 3), device=cuda)
    M = [np.eye(3)]
    for row in [(0, 5, 7, 8, 11), (0, 5, 7, 9, 8), (1, 5, 7, 8, 8), (0, 5, 8, 8, 8), (0, 5, 7, 0, 8), (0, 5, 7, 8, 0)]:
        with pytest.raises(RuntimeError):        # wider / taller than the slot, past the staging buffer, empty target
            N.image_batch_warp_resize_normalize(staging, [row], M, batch, 1)
    good = (0, 5, 7, 8, 8)
    for interp, border in [(2, 1), (-1, 1), (1, 4), (1, -1)]:
        with pytest.raises(RuntimeError):
            N.image_batch_warp_resize_normalize(staging, [good], M, batch, 1, interp, border)
    with pytest.raises(ValueError):              # a matrix per table row
        N.image_batch_warp_resize_normalize(staging, [good], [], batch, 1)
    batch.fill_(float("nan"))
    N.image_batch_warp_resize_normalize(staging, [good], M, batch, 1)
    torch.cuda.synchronize()
    assert not torch.isnan(batch).any()


# ------------------------------------------------------------------------------------------ the two routes
def _transforms(seed):
    """The --random-transform ranges of bin/train.py."""
    from batchai_retinanet_horovod_coco_amd.data.transform import random_transform_generator
    return random_transform_generator(
        prng=np.random.RandomState(seed), min_rotation=-0.1, max_rotation=0.1, min_translation=(-0.1, -0.1),
        max_translation=(0.1, 0.1), min_shear=-0.1, max_shear=0.1, min_scaling=(0.9, 0.9), max_scaling=(1.1, 1.1),
        flip_x_chance=0.5, flip_y_chance=0.5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_device_preprocessor_routes_equal(cuda, tmp_path, monkeypatch, dtype):
    """Four consecutive batches of the JPEG fixture (both staging buffers used and reused) with random transforms:
    the one-launch route and the per-image route give the same bits."""
    from batchai_retinanet_horovod_coco_amd.data import device_preprocess as dp
    from batchai_retinanet_horovod_coco_amd.data.transform import adjust_transform_for_image
    assert dp.TRAIN_FUSED is True
    gen = make_generator(write_fixture(tmp_path))
    params = gen.transform_parameters
    tg = _transforms(11)
    work = []
    for idx in ([0, 1, 2], [3, 4, 5, 6], [7, 8, 9], [0, 4]):
        images = [gen.load_image(i) for i in idx]
        mats = [adjust_transform_for_image(next(tg), im, params.relative_translation) for im in images]
        mats[-1] = None
        work.append((images, mats))
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(dp, "TRAIN_FUSED", fused)
        pre = dp.DevicePreprocessor(cuda, MIN_SIDE, MAX_SIDE, "caffe", dtype, pad_multiple=32)
        out[fused] = [pre(images, mats, 4, params) for images, mats in work]
        torch.cuda.synchronize()
    for a, b in zip(out[True], out[False]):
        assert a.shape == b.shape and a.shape[0] == 4 and a.shape[1] % 32 == 0 and a.shape[2] % 32 == 0
        assert a.dtype == dtype and torch.equal(_bits(a), _bits(b))
        assert a[0].float().abs().sum() > 0


def _loader_batches(root, fused, monkeypatch, dtype, slot_mb=0.0, n=5):
    from batchai_retinanet_horovod_coco_amd.data import device_preprocess as dp
    from batchai_retinanet_horovod_coco_amd.data import process_loader
    from batchai_retinanet_horovod_coco_amd.data.coco import CocoGenerator
    monkeypatch.setattr(dp, "TRAIN_FUSED", fused)
    dev = torch.device("cuda")
    g = CocoGenerator(str(root), "val2017", image_min_side=MIN_SIDE, image_max_side=MAX_SIDE, batch_size=3,
                      transform_generator=_transforms(7), seed=3, pad_multiple=32)
    g.device_preprocessor = dp.DevicePreprocessor(dev, MIN_SIDE, MAX_SIDE, "caffe", dtype, pad_multiple=32)
    assert process_loader.prestart()
    enq = process_loader.ProcessEnqueuer(g, workers=2, max_queue_size=2, device=dev, slot_mb=slot_mb).start()
    try:
        got = [enq.get() for _ in range(n)]
        torch.cuda.synchronize()
    finally:
        enq.stop()
    return got, dict(enq.stats)


@pytest.mark.parametrize("slot_mb,dtype", [(0.0, torch.float32), (0.0, torch.bfloat16), (0.08, torch.float32)],
                         ids=["arena-fp32", "arena-bf16", "inline-fp32"])
def test_process_loader_routes_equal(cuda, tmp_path, monkeypatch, slot_mb, dtype):
    """The process loader over the JPEG fixture with the switch on and off, same seed, 2 workers: every batch equal.
    A slot of 0.08 MiB (82.5 KiB) holds two of the three 36 KiB images of a batch of 96x128 or 128x96 ones, so the
    third goes through the pipe and is appended by the second copy (the loader prefetches past the batches read, so
    the count itself differs from run to run)."""
    root = write_fixture(tmp_path)
    got, stats = _loader_batches(root, True, monkeypatch, dtype, slot_mb)
    want, stats0 = _loader_batches(root, False, monkeypatch, dtype, slot_mb)
    for st in (stats, stats0):
        assert (st["inline_images"] > 0) == (slot_mb > 0)
    for a, b in zip(got, want):
        assert a["images"].dtype == dtype and torch.equal(_bits(a["images"]), _bits(b["images"]))
        assert a["images"][0].float().abs().sum() > 0
        for k in ("gt", "gt_count", "image_hw"):
            assert torch.equal(a[k], b[k])
