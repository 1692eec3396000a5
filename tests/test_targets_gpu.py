"""The anchor-target kernel (csrc/kernels/targets.hip) against the float64 numpy restatement of the reference
(``ops.anchors.anchor_targets_bbox`` / ``compute_overlap``), per image and per anchor, on the
values the kernel receives: the fp32 anchors, their centres rounded down to fp32, fp32 boxes with integer corners.

Shapes: the 15,354 anchors of a 256 x 320 padded image (15,354 % 256 = 250: the last block is partial) and
12 / 300 / 513 boxes, i.e. one, two and three LDS tiles of 256 boxes, the last of them holding a single box.
"""
import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import anchors as A
from batchai_retinanet_horovod_coco_amd.ops import native as N

pytestmark = pytest.mark.gpu

PAD_HW = (256, 320)
NUM_CLASSES = 80
# The kernel's fp32 IoU of these inputs differs from the float64 one by at most 9.3e-7 (emulated on the CPU for
# 12 / 300 / 513 boxes); 4x that decides which comparisons of two IoUs, or of an IoU with a threshold, an
# fp32 kernel is free to get either way.
IOU_EPS = 4e-6
MAX_EXCUSED = 8
# fp32 division and a multiply by 5 on values up to a few tens
REG_RTOL = 1e-5

# seeds whose boxes leave no anchor's best float64 IoU within 1e-5 of a threshold (nothing is excused below)
SEEDS = {12: 112, 300: 408, 513: 619, "duplicates": 632}

_ANCHORS = {}


def _anchors():
    """(fp32 anchors, the same in float64, centres rounded down to fp32) -- computed once, never modified."""
    if not _ANCHORS:
        a32 = A.anchors_for_shape(PAD_HW).astype(np.float32)
        a64 = a32.astype(np.float64)
        _ANCHORS["v"] = (a32, a64, A.centers_round_down(a64))
        assert a32.shape[0] == 15354 and a32.shape[0] % 256 == 250
    return _ANCHORS["v"]


def _boxes(rng, n, hw):
    """n boxes [x1, y1, x2, y2, label] with integer corners inside an image of (H, W) = hw."""
    H, W = hw
    w = rng.randint(6, 160, size=n)
    h = rng.randint(6, 160, size=n)
    x1 = (rng.rand(n) * (W - 1 - np.minimum(w, W - 2))).astype(np.int64)
    y1 = (rng.rand(n) * (H - 1 - np.minimum(h, H - 2))).astype(np.int64)
    x2 = np.minimum(x1 + w, W - 1)
    y2 = np.minimum(y1 + h, H - 1)
    out = np.stack([x1, y1, x2, y2, rng.randint(0, NUM_CLASSES, size=n)], axis=1).astype(np.float64)
    assert (out[:, 0] >= 0).all() and (out[:, 1] >= 0).all() and (out[:, 2] > out[:, 0]).all() \
        and (out[:, 3] > out[:, 1]).all()
    return out


def _batch(rng, G, counts, hws):
    """(B, G, 5) boxes; the rows from counts[b] on are large valid-looking boxes the kernel must not read."""
    gt = np.zeros((len(counts), G, 5))
    for b, (c, hw) in enumerate(zip(counts, hws)):
        gt[b, :c] = _boxes(rng, c, hw)
        gt[b, c:] = [0, 0, hw[1] - 1, hw[0] - 1, NUM_CLASSES - 1]
        gt[b, c::2] = [16, 16, 150, 120, 3]
    return gt


def _check(cuda, gt, counts, hws):
    """Run the kernel on the batch and compare every image with the float64 reference; returns the kernel's
    outputs and the reference's (arg, best IoU) per image."""
    a32, a64, c32 = _anchors()
    An = a32.shape[0]
    B, G = gt.shape[0], gt.shape[1]
    state, label, reg, npos = N.anchor_targets(
        torch.from_numpy(a32).to(cuda), torch.from_numpy(gt).float().to(cuda),
        torch.tensor(counts, dtype=torch.int32, device=cuda), torch.tensor(hws, dtype=torch.int32, device=cuda),
        centers=torch.from_numpy(c32).to(cuda))
    torch.cuda.synchronize()
    assert state.shape == (B, An) and label.shape == (B, An) and reg.shape == (B, An, 4)
    state, label, reg = state.cpu().numpy(), label.cpu().numpy(), reg.cpu().numpy().astype(np.float64)
    assert npos.item() == int((state == 1).sum())
    assert gt.astype(np.float32).astype(np.float64).tolist() == gt.tolist()       # the kernel sees these values
    ref_pos, refs = 0, []
    for b in range(B):
        ann = gt[b, :counts[b]]
        r_onehot, r_reg, r_state = A.anchor_targets_bbox(PAD_HW, ann, NUM_CLASSES, mask_shape=hws[b], anchors=a64)
        inside = ~((c32[:, 0] >= hws[b][1]) | (c32[:, 1] >= hws[b][0]))
        assert ((r_state == -1) | inside).all() and 0 < inside.sum()
        if counts[b] == 0:
            assert (r_state[inside] == 0).all()
            assert (state[b] == r_state).all()
            assert (label[b] == 0).all() and (reg[b] == 0).all()
            refs.append((None, None))
            continue
        ov = A.compute_overlap(a64, ann[:, :4])
        arg = ov.argmax(axis=1)
        top = np.sort(np.partition(ov, -2, axis=1)[:, -2:], axis=1) if counts[b] > 1 else \
            np.concatenate([np.full((An, 1), -1.0), ov], axis=1)
        best, second = top[:, 1], top[:, 0]
        assert (best == ov[np.arange(An), arg]).all()
        # an IoU within IOU_EPS of a threshold may land on either side in fp32: excused, but there are few
        excused = (np.abs(best - A.NEGATIVE_OVERLAP) <= IOU_EPS) | (np.abs(best - A.POSITIVE_OVERLAP) <= IOU_EPS)
        print("image {}: {} boxes, {} positive, {} ignored, {} excused".format(
            b, counts[b], int((r_state == 1).sum()), int((r_state == -1).sum()), int(excused.sum())))
        assert excused.sum() <= MAX_EXCUSED
        keep = ~excused
        bad = keep & (state[b] != r_state)
        assert not bad.any(), ("state", b, np.nonzero(bad)[0][:8], state[b][bad][:8], r_state[bad][:8], best[bad][:8])
        ref_pos += int((r_state[keep] == 1).sum())
        assert int((state[b][keep] == 1).sum()) == int((r_state[keep] == 1).sum())
        # the match: wherever the argmax is decided (or an exact tie, where the first index wins)
        clear = keep & ((best - second > IOU_EPS) | (best == second))
        assert clear.sum() > 0.95 * An
        r_label = ann[arg, 4].astype(np.int64)
        bad = clear & (label[b] != r_label)
        assert not bad.any(), ("label", b, np.nonzero(bad)[0][:8], label[b][bad][:8], r_label[bad][:8], arg[bad][:8])
        pos = clear & (r_state == 1)
        assert (r_onehot[pos].argmax(axis=1) == label[b][pos]).all() and (r_onehot[pos].sum(axis=1) == 1).all()
        err = np.abs(reg[b] - r_reg)
        bad = clear[:, None] & (err > REG_RTOL * np.maximum(1.0, np.abs(r_reg)))
        assert not bad.any(), ("regression", b, np.nonzero(bad)[0][:8], reg[b][bad][:8], r_reg[bad][:8])
        refs.append((arg, best))
    return state, label, reg, refs


@pytest.mark.parametrize("G", [12, 300, 513])
def test_anchor_targets_tiles(cuda, G):
    """One, two and three LDS tiles; per-image counts of G, 0 and G // 2 in one batch; an image as large as the
    padding and two of (200, 300) inside it; a box equal to an anchor rounded to integers and a box covering
    the whole image."""
    rng = np.random.RandomState(SEEDS[G])
    counts = [G, 0, G // 2]
    hws = [PAD_HW, (200, 300), (200, 300)]
    gt = _batch(rng, G, counts, hws)
    _, a64, _ = _anchors()
    inside = np.nonzero((a64[:, 0] >= 0) & (a64[:, 1] >= 0) & (a64[:, 2] <= 299) & (a64[:, 3] <= 199))[0]
    for b in (0, 2):
        gt[b, 1, :4] = np.round(a64[inside[len(inside) // 2 + b]])
        gt[b, counts[b] - 1, :4] = [0, 0, hws[b][1] - 1, hws[b][0] - 1]     # the last box of the last tile
    state, _, _, refs = _check(cuda, gt, counts, hws)
    for b in (0, 2):
        assert (state[b] == 1).sum() > 50 and (state[b] == 0).sum() > 50
        assert refs[b][1].max() > 0.9                                         # the anchor-shaped box is matched
    # anchors centred at or beyond (200, 300) are ignored in the smaller images, and some anchors are
    assert (state[2] == -1).sum() > (state[0] == -1).sum() + 1000


def test_anchor_targets_duplicates_first_wins(cuda):
    """The same box under two labels at j < k, j in the first LDS tile and k in the second (and a pair across
    the second and third): every anchor they match best takes label j -- the first maximum wins across tiles."""
    G = 513
    rng = np.random.RandomState(SEEDS["duplicates"])
    counts, hws = [G, G, 300], [PAD_HW, PAD_HW, (200, 300)]
    gt = _batch(rng, G, counts, hws)
    pairs = {0: [(5, 256), (255, 511), (300, 512)], 1: [(0, 257), (100, 400)], 2: [(17, 299), (200, 256)]}
    for b, pp in pairs.items():
        for j, k in pp:
            gt[b, k, :4] = gt[b, j, :4]
            gt[b, k, 4] = (gt[b, j, 4] + 1 + (j % 7)) % NUM_CLASSES
            assert gt[b, k, 4] != gt[b, j, 4]
    _, label, _, refs = _check(cuda, gt, counts, hws)
    for b, pp in pairs.items():
        arg, best = refs[b]
        matched = 0
        for j, k in pp:
            m = (arg == j) & (best > 0)
            matched += int(m.sum())
            assert (label[b][m] == int(gt[b, j, 4])).all()
            assert not (arg == k).any()
        assert matched >= 10


def test_anchor_targets_no_boxes(cuda):
    """B = 1 with gt_count = 0: every inside anchor negative, npos 0, label 0, regression exactly 0."""
    rng = np.random.RandomState(9)
    gt = _batch(rng, 12, [0], [(200, 300)])
    state, label, reg, _ = _check(cuda, gt, [0], [(200, 300)])
    assert (state == 1).sum() == 0 and (state == 0).sum() > 5000 and (state == -1).sum() > 1000
    assert not label.any() and not reg.any()
