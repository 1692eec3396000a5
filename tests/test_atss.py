"""ATSS target assignment on the CPU: the float64 oracle of ``ops/anchors.py`` on hand-made cases, the fp32 torch
form against it, the window rule of the HIP kernel (its Python mirror against brute force), ``Trainer(assigner=...)``,
what checkpoints record and the two flags of ``train.py``.

Geometry: the 15,354 anchors of a 256 x 320 padded image, levels 32x40, 16x20, 8x10, 4x5 and 2x3 (strides 8..128)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.bin import train as T
from batchai_retinanet_horovod_coco_amd.io import checkpoint
from batchai_retinanet_horovod_coco_amd.ops import anchors as A

PAD = (256, 320)
C = 7
ANCHORS = A.anchors_for_shape(PAD)
LEVELS = A.level_table(PAD)
GRID = [(32, 40, 8), (16, 20, 16), (8, 10, 32), (4, 5, 64), (2, 3, 128)]


def _ann(*rows):
    return np.asarray(rows, dtype=np.float64).reshape(-1, 5)


def _targets(ann, topk=9, mask=None):
    return A.atss_targets_bbox(PAD, ann, C, mask_shape=mask, topk=topk, anchors=ANCHORS)


# ------------------------------------------------------------------------------------------------ the oracle by hand
def _iou(a, g):
    iw = min(a[2], g[2]) - max(a[0], g[0]) + 1
    ih = min(a[3], g[3]) - max(a[1], g[1]) + 1
    if iw <= 0 or ih <= 0:
        return 0.0
    return iw * ih / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (g[2] - g[0] + 1) * (g[3] - g[1] + 1) - iw * ih)


def _by_hand(box, topk=9):
    """Candidates and threshold of one box with plain loops: [(anchor index, IoU, grid centre inside)], threshold."""
    gcx, gcy = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
    cand, first = [], 0
    for h, w, s in GRID:
        cells = sorted((((ix + 0.5) * s - gcx) ** 2 + ((iy + 0.5) * s - gcy) ** 2, iy * w + ix)
                       for iy in range(h) for ix in range(w))
        for _, loc in cells[:topk]:
            cx, cy = (loc % w + 0.5) * s, (loc // w + 0.5) * s
            inside = min(cx - box[0], cy - box[1], box[2] - cx, box[3] - cy) > 0.01
            cand += [(first + loc * 9 + j, _iou(ANCHORS[first + loc * 9 + j], box), inside) for j in range(9)]
        first += h * w * 9
    v = [c[1] for c in cand]
    mean = sum(v) / len(v)
    std = math.sqrt(sum((x - mean) ** 2 for x in v) / (len(v) - 1)) if len(v) > 1 else 0.0
    return cand, mean + std


def test_level_table():
    assert LEVELS.tolist() == [[0, 32, 40, 8], [11520, 16, 20, 16], [14400, 8, 10, 32], [15120, 4, 5, 64],
                               [15300, 2, 3, 128]]
    assert ANCHORS.shape[0] == 15354
    cache = A.AnchorCache()
    assert (cache.levels(PAD, torch.device("cpu")) == LEVELS).all()
    assert cache.levels(PAD, torch.device("cpu")) is cache.levels(PAD, "cpu", None)
    # the grid centres of the table are the anchors' centres (up to the rounding of the anchor sum)
    for first, h, w, s in LEVELS.tolist():
        loc = np.arange(h * w)
        cx = (ANCHORS[first + loc * 9, 0] + ANCHORS[first + loc * 9, 2]) / 2
        assert np.abs(cx - (loc % w + 0.5) * s).max() < 1e-9
    with pytest.raises(ValueError, match="add up"):
        A.atss_assign(ANCHORS[:-9], LEVELS, np.zeros((0, 4)))


def test_box_equal_to_an_anchor():
    i = 14400 + (3 * 10 + 4) * 9 + 4                     # level of stride 32, location (4, 3), the square anchor
    box = np.round(ANCHORS[i])
    r = A.atss_assign(ANCHORS, LEVELS, box[None], 9)
    cand, thr = _by_hand(box)
    assert len(cand) == (9 + 9 + 9 + 9 + 6) * 9 == r["candidates"].shape[1]
    assert r["candidates"][0].tolist() == [c[0] for c in cand]
    assert np.abs(r["iou"][0] - np.array([c[1] for c in cand])).max() < 1e-15
    assert abs(r["threshold"][0] - thr) < 1e-14 and 0.2 < thr < 0.9
    assert r["arg"][i] == 0 and r["best"][i] > 0.95
    want = sorted(c[0] for c in cand if c[2] and c[1] >= thr)
    assert np.nonzero(r["arg"] == 0)[0].tolist() == want and len(want) >= 1
    labels, reg, state = _targets(_ann([*box, 5]))
    assert np.nonzero(state == 1)[0].tolist() == want
    assert (labels[want, 5] == 1).all() and labels[state >= 0].sum() == len(want)
    assert np.allclose(reg[i], (box - ANCHORS[i]) / np.tile(ANCHORS[i, 2:] - ANCHORS[i, :2], 2) / 0.2)
    off = np.ones(len(state), dtype=bool)
    off[want] = False
    assert not reg[off].any()                              # exactly 0 off the positives: there is no ignore band
    # (the 2 x 3 level's last column is centred at x = 320, on the edge of the padded shape: outside, as ever)
    assert set(np.unique(state)) == {-1.0, 0.0, 1.0} and (state == -1).sum() == 2 * 9


def test_centre_on_a_cell_boundary_takes_the_lower_index():
    box = [50, 40, 110, 120]                               # centre (80, 80): x1 + x2 = 16 * 10
    r = A.atss_assign(ANCHORS, LEVELS, np.array([box], dtype=np.float64), 9)
    assert r["selected"][0, 0, :4].tolist() == [9 * 40 + 9, 9 * 40 + 10, 10 * 40 + 9, 10 * 40 + 10]
    assert r["selected"][0, 1, :4].tolist() == [4 * 20 + 4, 4 * 20 + 5, 5 * 20 + 4, 5 * 20 + 5]
    assert r["selected"][0, 2, 0] == 2 * 10 + 2            # a grid centre of the stride-32 level
    one = A.atss_assign(ANCHORS, LEVELS, np.array([box], dtype=np.float64), 1)
    assert one["selected"][0, :, 0].tolist() == [369, 84, 22, 6, 0]
    assert r["candidates"][0].tolist() == [c[0] for c in _by_hand(box)[0]]


@pytest.mark.parametrize("box", [[0, 0, 37, 29], [283, 227, 319, 255], [0, 200, 50, 255]])
def test_box_at_a_corner(box):
    r = A.atss_assign(ANCHORS, LEVELS, np.array([box], dtype=np.float64), 9)
    cand, thr = _by_hand(box)
    assert r["candidates"][0].tolist() == [c[0] for c in cand] and abs(r["threshold"][0] - thr) < 1e-14
    assert (r["selected"][0, :4] >= 0).all() and (r["selected"][0, 4, 6:] == -1).all()
    assert sorted(r["selected"][0, 4, :6].tolist()) == list(range(6))
    assert (r["arg"] == 0).sum() >= 1


def test_box_too_small_for_a_grid_centre():
    others = _ann([30, 40, 130, 150, 1], [150, 20, 280, 200, 2])
    tiny = [101, 101, 103, 103, 3]                          # grid centres are at 4 + 8 i
    base = _targets(others)
    for ann in (np.concatenate([others, _ann(tiny)]), np.concatenate([_ann(tiny), others])):
        got = _targets(ann)
        for x, y in zip(base, got):
            assert np.array_equal(x, y)
    alone = _targets(_ann(tiny))
    assert not alone[0][alone[2] >= 0].any() and not alone[1].any() and not (alone[2] == 1).any()
    assert (base[2] == 1).sum() > 10


def test_shared_anchor_goes_to_the_larger_iou():
    a, b = [60.0, 50, 180, 170, 1], [66.0, 54, 190, 172, 2]
    ra = A.atss_assign(ANCHORS, LEVELS, _ann(a), 9)
    rb = A.atss_assign(ANCHORS, LEVELS, _ann(b), 9)
    both = A.atss_assign(ANCHORS, LEVELS, _ann(a, b), 9)
    shared = np.nonzero((ra["arg"] == 0) & (rb["arg"] == 0))[0]
    assert len(shared) >= 4
    to_b = rb["best"][shared] > ra["best"][shared]
    assert to_b.any() and (~to_b).any()
    assert (both["arg"][shared] == to_b.astype(int)).all()
    assert (both["best"][shared] == np.maximum(ra["best"], rb["best"])[shared]).all()
    labels = _targets(_ann(a, b))[0]
    assert (labels[shared].argmax(1) == np.where(to_b, 2, 1)).all() and (labels[shared].sum(1) == 1).all()
    # in the other order the same boxes win
    swapped = A.atss_assign(ANCHORS, LEVELS, _ann(b, a), 9)
    assert (swapped["arg"][shared] == 1 - to_b.astype(int)).all()


def test_duplicates_first_wins_and_no_boxes():
    box = [40, 30, 200, 180]
    labels, reg, state = _targets(_ann([*box, 4], [*box, 6], [*box, 1]))
    pos = state == 1
    assert pos.sum() > 10 and (labels[pos, 4] == 1).all() and not (labels[:, 6] == 1).any() \
        and not (labels[:, 1] == 1).any()
    labels, reg, state = _targets(np.zeros((0, 5)))
    assert not labels[state >= 0].any() and not reg.any() and (state == -1).sum() == 18 and not (state == 1).any()
    labels, reg, state = _targets(np.zeros((0, 5)), mask=(200, 300))
    assert set(np.unique(state)) == {-1.0, 0.0} and (labels[state == -1] == -1).all() and not reg.any()


def test_image_smaller_than_the_padding():
    ann = _ann([30, 40, 130, 150, 1], [283, 150, 319, 255, 2], [283, 227, 319, 255, 3])
    full = _targets(ann)
    small = _targets(ann, mask=(200, 300))
    cx, cy = (ANCHORS[:, 0] + ANCHORS[:, 2]) / 2, (ANCHORS[:, 1] + ANCHORS[:, 3]) / 2
    outside = (cx >= 300) | (cy >= 200)
    assert (small[2][outside] == -1).all() and (small[0][outside] == -1).all()
    assert np.array_equal(small[2][~outside], full[2][~outside]) and np.array_equal(small[1], full[1])
    lost = outside & (full[2] == 1)
    assert lost.sum() >= 2 and (full[2][~outside] == 1).sum() > 5
    assert (full[0][lost].argmax(1) >= 2).all()


@pytest.mark.parametrize("topk,count", [(1, 45), (16, (16 * 4 + 6) * 9)])
def test_topk(topk, count):
    box = [70, 60, 170, 190]
    r = A.atss_assign(ANCHORS, LEVELS, np.array([box], dtype=np.float64), topk)
    cand, thr = _by_hand(box, topk)
    assert len(cand) == count and r["candidates"][0].tolist() == [c[0] for c in cand]
    assert abs(r["threshold"][0] - thr) < 1e-14
    assert (_targets(_ann([*box, 0]), topk=topk)[2] == 1).sum() == sum(c[2] and c[1] >= thr for c in cand) >= 1


def test_topk_range():
    for k in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="topk"):
            _targets(_ann([70, 60, 170, 190, 0]), topk=k)
    # a single candidate has no deviation: the threshold is its IoU
    one = np.array([[0, 0, 15, 15]], dtype=np.float64)
    r = A.atss_assign(one, [[0, 1, 1, 16]], np.array([[2.0, 2, 13, 13]]), 1)
    assert r["threshold"][0] == r["iou"][0, 0] and r["arg"][0] == 0


def test_generator_takes_the_oracle():
    from batchai_retinanet_horovod_coco_amd.data.synthetic import SyntheticGenerator
    g = SyntheticGenerator(num_images=2, height=64, width=96, num_classes=3, max_boxes=3, batch_size=2,
                           compute_anchor_targets=A.atss_targets_bbox)
    imgs, anns = [np.zeros((64, 96, 3), np.float32)] * 2, [_ann([10, 10, 50, 40, 1]), np.zeros((0, 5))]
    reg, lab = g.compute_targets(imgs, anns)
    assert reg.shape[-1] == 5 and lab.shape[-1] == 4 and (lab[0, :, -1] == 1).sum() >= 1 and not (lab[1, :, -1] == 1).any()


# ------------------------------------------------------------------------------------------------ the torch form
def _random_boxes(rng, n):
    w, h = rng.randint(6, 160, n), rng.randint(6, 160, n)
    x1, y1 = (rng.rand(n) * (318 - np.minimum(w, 317))).astype(np.int64), (rng.rand(n) * (254 - np.minimum(h, 253))).astype(np.int64)
    return np.stack([x1, y1, np.minimum(x1 + w, 319), np.minimum(y1 + h, 255), rng.randint(0, C, n)], 1).astype(np.float64)


@pytest.mark.parametrize("topk", [1, 9, 16])
def test_torch_form_against_the_oracle(topk):
    rng = np.random.RandomState(3 + topk)
    G, counts, hws = 40, [40, 0, 17], [PAD, (200, 300), (200, 300)]
    gt = np.full((3, G, 5), np.nan)                        # rows past the count are never used
    for b, c in enumerate(counts):
        gt[b, :c] = _random_boxes(rng, c)
    a32 = ANCHORS.astype(np.float32)
    a64 = a32.astype(np.float64)
    c32 = A.centers_round_down(a64)
    state, label, reg, thr, sel = A.atss_targets_torch(
        torch.from_numpy(a32), LEVELS, torch.from_numpy(gt).float(), torch.tensor(counts), torch.tensor(hws), topk=topk,
        centers=torch.from_numpy(c32), return_aux=True)
    assert state.dtype == torch.int8 and label.dtype == torch.int32 and reg.dtype == torch.float32
    plain = A.atss_targets_torch(torch.from_numpy(a32), LEVELS, torch.from_numpy(gt).float(), torch.tensor(counts),
                                 torch.tensor(hws), topk=topk)
    assert torch.equal(plain[0], state) and torch.equal(plain[1], label) and torch.equal(plain[2], reg)
    state, label, reg, thr, sel = (t.numpy() for t in (state, label, reg, thr, sel))
    eps = 1e-6
    for b, c in enumerate(counts):
        assert np.isinf(thr[b, c:]).all() and (sel[b, c:] == -1).all()
        labels, r_reg, r_state = A.atss_targets_bbox(PAD, gt[b, :c], C, mask_shape=hws[b], topk=topk, anchors=a64)
        if c == 0:
            assert np.array_equal(state[b], r_state) and not label[b].any() and not reg[b].any()
            continue
        r = A.atss_assign(a64, LEVELS, gt[b, :c], topk)
        # integer corners: the distances are exact in fp32, so the candidate sets are the oracle's
        assert np.array_equal(sel[b, :c], r["selected"])
        assert np.abs(thr[b, :c] - r["threshold"]).max() < eps
        near = np.zeros(len(a64), dtype=bool)
        for g in range(c):
            near[r["candidates"][g][r["inside"][g] & (np.abs(r["iou"][g] - r["threshold"][g]) <= eps)]] = True
        assert near.sum() <= 8
        assert np.array_equal(state[b][~near], r_state[~near])
        pos = (r["arg"] >= 0) & ~near
        assert pos.sum() > 20 and (label[b][pos] == gt[b, r["arg"][pos], 4]).all()
        assert np.abs(reg[b][~near] - r_reg[~near]).max() < 1e-4
        assert not reg[b][~near & (r["arg"] < 0)].any() and not label[b][~near & (r["arg"] < 0)].any()


def test_torch_form_without_box_rows():
    a32 = torch.from_numpy(ANCHORS.astype(np.float32))
    state, label, reg, thr, sel = A.atss_targets_torch(a32, LEVELS, torch.zeros(2, 0, 5), torch.zeros(2, dtype=torch.int32),
                                                       torch.tensor([PAD, (200, 300)]), return_aux=True,
                                                       centers=torch.from_numpy(A.centers_round_down(ANCHORS)))
    assert thr.shape == (2, 0) and sel.shape == (2, 0, 5, 9)
    assert set(state.unique().tolist()) == {-1, 0} and not label.any() and not reg.any()
    assert int((state[0] == -1).sum()) == 18 and int((state[1] == -1).sum()) > 1000


# ------------------------------------------------------------------------------------------------ the window rule
@pytest.mark.parametrize("h,w", [(8, 10), (2, 3), (1, 24), (3, 17)])
def test_window_rule_against_brute_force(h, w):
    """Every half-integer centre of the grid (stride 4: eighths of a cell, so cell centres, edges and corners and
    their ties all occur) and every K: the K nearest inside the kernel's window, found in fp32, are the K nearest of
    the whole level in float64; the long thin grids make the window fall back to the whole level."""
    s = 4
    full = windowed = 0
    for gy2 in range(0, 2 * h * s + 1):
        for gx2 in range(0, 2 * w * s + 1):
            gcx, gcy = gx2 / 2, gy2 / 2
            order = A._nearest_locations(h, w, s, gcx, gcy, 16)
            for K in range(1, 17):
                rect = A.atss_window(h, w, s, gcx, gcy, K)
                if rect == (0, w - 1, 0, h - 1):
                    full += 1
                    continue                                  # the whole level: brute force itself
                windowed += 1
                got = A._nearest_locations(h, w, s, gcx, gcy, K, rect=rect, dtype=np.float32)
                assert got.tolist() == order[:K].tolist(), (gcx, gcy, K, rect)
    assert full > 0 and (windowed > 0 or h * w <= 25)


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(seed=0, **kw):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    torch.manual_seed(seed)
    model = models.backbone("resnet18").retinanet(3)
    return Trainer(model, lr=1e-3, clipnorm=0.0, device=torch.device("cpu"), **kw)


def _batch():
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    return make_batch(2, 64, 96, num_classes=3, max_boxes=3, generator=torch.Generator().manual_seed(5))


def test_trainer_trains_with_atss():
    tr = _trainer(assigner="atss")
    b = _batch()
    state, label, reg, npos = tr.compute_targets(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    assert npos.item() == int((state == 1).sum()) > 0 and not bool((state == -1).any() and False)
    assert not reg[state == 0].any() and not label[state == 0].any()
    for i in range(2):
        n = int(b["gt_count"][i])
        ref = A.atss_targets_bbox((64, 96), b["gt"][i, :n].double().numpy(), 3, mask_shape=b["image_hw"][i].tolist())
        assert (state[i].numpy() == ref[2]).mean() > 0.999
    w0 = tr.flat.data.clone()
    for _ in range(3):
        logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
        assert all(math.isfinite(float(v)) for v in logs.values())
    assert float(logs["regression_loss"]) > 0 and not torch.equal(w0, tr.flat.data)
    other = _trainer().compute_targets(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    assert not torch.equal(other[0], state)
    k1 = _trainer(assigner="atss", atss_topk=1).compute_targets(b["images"], b["gt"], b["gt_count"], b["image_hw"])
    assert not torch.equal(k1[0], state)


def test_naming_iou_changes_nothing():
    b = _batch()
    runs = []
    for kw in ({}, {"assigner": "iou"}):
        tr = _trainer(**kw)
        for _ in range(2):
            logs = tr.train_on_batch(b["images"], b["gt"], b["gt_count"], b["image_hw"])
        runs.append((tr.flat.data.clone(), float(logs["loss"])))
        assert tr.assigner == "iou" and not hasattr(tr.base_optimizer, "assigner")
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_trainer_argument_checks():
    with pytest.raises(ValueError, match="assigner"):
        _trainer(assigner="fcos")
    with pytest.raises(ValueError, match="atss_topk"):
        _trainer(atss_topk=5)
    with pytest.raises(ValueError, match="topk"):
        _trainer(assigner="atss", atss_topk=17)


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("ext", ["h5", "safetensors"])
def test_checkpoint_records_the_assigner(tmp_path, ext):
    for topk in (9, 5):
        tr = _trainer(assigner="atss", atss_topk=topk)
        cfg = checkpoint.training_config(tr.base_optimizer)
        assert cfg["assigner"] == "atss" and cfg.get("atss_topk") == (None if topk == 9 else topk)
        path = str(tmp_path / "atss{}.{}".format(topk, ext))
        checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
        assert checkpoint.stored_assigner(path) == "atss" and checkpoint.stored_atss_topk(path) == topk
        assert checkpoint.stored_regression_loss(path) == "smooth_l1"
    plain = _trainer()
    path = str(tmp_path / ("plain." + ext))
    checkpoint.save_checkpoint(path, plain.model, plain.base_optimizer, epoch=1)
    assert checkpoint.stored_assigner(path) == "iou" and checkpoint.stored_atss_topk(path) == 9
    weights_only = str(tmp_path / ("weights." + ext))
    checkpoint.save_checkpoint(weights_only, plain.model, None)
    assert checkpoint.stored_assigner(weights_only) is None


def test_default_training_config_is_unchanged():
    """Without the new arguments the stored training_config is, byte for byte, the one written before they existed."""
    for tr in (_trainer(), _trainer(assigner="iou")):
        opt = tr.base_optimizer
        before = json.dumps({"optimizer_config": {"class_name": "Adam", "config": opt.get_config()},
                             "loss": {"regression": "_smooth_l1", "classification": "_focal"},
                             "metrics": [], "sample_weight_mode": None, "loss_weights": None})
        assert json.dumps(checkpoint.training_config(opt)) == before


# ------------------------------------------------------------------------------------------------ CLI
def test_flags_parse():
    a = T.parse_args(["coco", "/x"])
    assert a.assigner == "iou" and a.atss_topk == 9
    a = T.parse_args(["--assigner", "atss", "coco", "/x"])
    assert (a.assigner, a.atss_topk) == ("atss", 9)
    a = T.parse_args(["--assigner", "atss", "--atss-topk", "12", "--regression-loss", "giou", "--optimizer", "sgd",
                      "--ema-decay", "0.99", "--graph", "coco", "/x"])
    assert (a.assigner, a.atss_topk, a.regression_loss, a.optimizer) == ("atss", 12, "giou", "sgd")
    assert T.build_parser().get_default("assigner") is None and T.build_parser().get_default("atss_topk") is None
    with pytest.raises(SystemExit):
        T.parse_args(["--assigner", "fcos", "coco", "/x"])
    with pytest.raises(SystemExit, match="atss-topk"):
        T.parse_args(["--atss-topk", "9", "coco", "/x"])
    with pytest.raises(SystemExit, match="atss-topk"):
        T.parse_args(["--assigner", "iou", "--atss-topk", "5", "coco", "/x"])
    for k in ("0", "17"):
        with pytest.raises(SystemExit, match="atss-topk"):
            T.parse_args(["--assigner", "atss", "--atss-topk", k, "coco", "/x"])
    assert "atss" in T.build_parser().format_help()


def test_flags_against_snapshot(tmp_path, recwarn):
    tr = _trainer(assigner="atss", atss_topk=5)
    path = str(tmp_path / "atss.h5")
    checkpoint.save_checkpoint(path, tr.model, tr.base_optimizer, epoch=1)
    a = T.parse_args(["--snapshot", path, "coco", "/x"])                     # the file decides
    assert (a.assigner, a.atss_topk) == ("atss", 5)
    a = T.parse_args(["--snapshot", path, "--assigner", "atss", "--atss-topk", "7", "coco", "/x"])
    assert (a.assigner, a.atss_topk) == ("atss", 7)
    a = T.parse_args(["--snapshot", path, "--assigner", "atss", "coco", "/x"])
    assert (a.assigner, a.atss_topk) == ("atss", 5)
    assert not [w for w in recwarn.list if "assigner" in str(w.message)]
    with pytest.warns(UserWarning, match="assigner iou differs.*atss"):       # the flag wins
        a = T.parse_args(["--snapshot", path, "--assigner", "iou", "coco", "/x"])
    assert (a.assigner, a.atss_topk) == ("iou", 9)
    plain = _trainer()
    path = str(tmp_path / "plain.h5")
    checkpoint.save_checkpoint(path, plain.model, plain.base_optimizer, epoch=1)
    assert T.parse_args(["--snapshot", path, "coco", "/x"]).assigner == "iou"
    with pytest.warns(UserWarning, match="assigner atss differs.*iou"):
        a = T.parse_args(["--snapshot", path, "--assigner", "atss", "coco", "/x"])
    assert (a.assigner, a.atss_topk) == ("atss", 9)
    with pytest.raises(SystemExit, match="atss-topk"):
        T.parse_args(["--snapshot", path, "--atss-topk", "5", "coco", "/x"])


def test_cli_trains_snapshots_and_resumes(tmp_path):
    common = ["--no-weights", "--backbone", "resnet18", "--batch-size", "2", "--image-min-side", "64",
              "--image-max-side", "96", "--snapshot-path", str(tmp_path / "snap"), "--tensorboard-dir", "",
              "--device", "cpu", "--workers", "1", "--seed", "1", "--no-evaluation", "--lr", "1e-4"]
    data = ["synthetic", "--num-images", "2", "--height", "64", "--width", "96", "--num-classes", "4", "--max-boxes", "3"]
    h = T.main(common + ["--assigner", "atss", "--atss-topk", "7", "--regression-loss", "giou", "--epochs", "1",
                         "--steps", "2"] + data)
    assert len(h.history["loss"]) == 1 and all(math.isfinite(v) for v in h.history["regression_loss"])
    ck = str(tmp_path / "snap" / "checkpoint-01.h5")
    assert os.path.exists(ck) and checkpoint.stored_assigner(ck) == "atss" and checkpoint.stored_atss_topk(ck) == 7
    assert checkpoint.stored_regression_loss(ck) == "giou"
    # resume without the flags: the snapshot says ATSS with 7, and the next snapshot says so again
    h2 = T.main(["--snapshot", ck] + common[1:] + ["--epochs", "2", "--steps", "1"] + data)
    assert h2.epoch == [1]
    ck2 = str(tmp_path / "snap" / "checkpoint-02.h5")
    assert checkpoint.stored_assigner(ck2) == "atss" and checkpoint.stored_atss_topk(ck2) == 7
