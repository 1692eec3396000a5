"""The ATSS kernels (csrc/kernels/targets.hip, ``mxr_atss_targets``) against the float64 oracle
(``ops.anchors.atss_assign`` / ``atss_targets_bbox``), per image, per box and per anchor, on the values the kernels
receive: the fp32 anchors, their centres rounded down to fp32, fp32 boxes with integer corners.

Geometry of test_targets_gpu.py: the 15,354 anchors of a 256 x 320 padded image (the last block of 256 is partial),
levels 32x40, 16x20, 8x10, 4x5 and 2x3 -- the last has 6 locations, fewer than topk = 9: "take all" -- and 12 / 300
boxes, one and two LDS tiles, with per-image counts [G, 0, G // 2].

THR_EPS: the kernel's fp32 arithmetic emulated on the CPU for these inputs (``_emulated_deviation``: the candidates'
IoUs in numpy float32, the mean and the two-sweep deviation of the fp32 torch form) differs from float64 by at most
2.2e-7 in an IoU (G = 300, topk = 9) and 7.2e-8 in a threshold (G = 300, topk = 1; the last digit moves with the
order in which the host's torch sums); 4x the larger is the band inside which an fp32 kernel may decide ``IoU >= threshold``, or order two IoUs, either way.  The
test recomputes the emulated maxima and refuses a larger one.  The seeds leave no candidate of the float64 oracle
within 1e-5 of its box's threshold, so nothing is excused.
"""
import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import anchors as A
from batchai_retinanet_horovod_coco_amd.ops import native as N

pytestmark = pytest.mark.gpu

PAD_HW = (256, 320)
NUM_CLASSES = 80
THR_EPS = 8.8e-7        # 4 x 2.2e-7, see above
MAX_EXCUSED = 8
REG_RTOL = 1e-5         # as test_targets_gpu.py: an fp32 division and a multiply by 5
MIN_MARGIN = 1e-5
# (G, topk) -> seed; every one confirmed against the oracle (the test asserts the margin again)
SEEDS = {(12, 1): 100, (12, 9): 100, (12, 16): 100, (300, 1): 110, (300, 9): 104, (300, 16): 115}

_CACHE = {}


def _anchors():
    """(fp32 anchors, the same in float64, centres rounded down to fp32, level table) -- computed once."""
    if "a" not in _CACHE:
        a32 = A.anchors_for_shape(PAD_HW).astype(np.float32)
        a64 = a32.astype(np.float64)
        lv = A.level_table(PAD_HW)
        assert a32.shape[0] == 15354 and a32.shape[0] % 256 == 250
        assert lv[:, 1:3].tolist() == [[32, 40], [16, 20], [8, 10], [4, 5], [2, 3]]
        _CACHE["a"] = (a32, a64, A.centers_round_down(a64), lv)
    return _CACHE["a"]


def _boxes(rng, n, hw):
    """n boxes [x1, y1, x2, y2, label] with integer corners inside an image of (H, W) = hw (test_targets_gpu.py's)."""
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


COUNTS = lambda G: [G, 0, G // 2]                                       # noqa: E731
HWS = [PAD_HW, (200, 300), (200, 300)]
# index of each special box within an image's rows (all below 6 = 12 // 2)
ANCHOR_BOX, CORNER, BOUNDARY, TINY, DUP = 0, 1, 2, 3, 4


def _batch(seed, G):
    """(B, G, 5) boxes; the rows from counts[b] on are large valid-looking boxes the kernels must not read.  Images
    0 and 2 hold, among the random boxes: a box equal to a rounded anchor, a box in the last corner of the padded
    area (the corner of image 0; beyond image 2, whose copy has all its positives centred outside: ignored), one whose
    centre sits on a cell boundary of every level up to stride 32, one too small for any grid centre, a duplicate of
    box DUP under another label in the last row (the second LDS tile when G = 300 in image 0) and, in the row
    before, a box covering the whole image."""
    rng = np.random.RandomState(seed)
    counts = COUNTS(G)
    _, a64, _, _ = _anchors()
    gt = np.zeros((len(counts), G, 5))
    inside = np.nonzero((a64[:, 0] >= 0) & (a64[:, 1] >= 0) & (a64[:, 2] <= 299) & (a64[:, 3] <= 199))[0]
    for b, (c, hw) in enumerate(zip(counts, HWS)):
        gt[b, :c] = _boxes(rng, c, hw)
        gt[b, c:] = [0, 0, hw[1] - 1, hw[0] - 1, NUM_CLASSES - 1]
        gt[b, c::2] = [16, 16, 150, 120, 3]
        if c:
            gt[b, ANCHOR_BOX, :4] = np.round(a64[inside[len(inside) // 2 + b]])
            gt[b, CORNER, :4] = [283, 227, 319, 255]              # centre (301, 241)
            gt[b, BOUNDARY, :4] = [50, 40, 110, 120]              # centre (80, 80): x1 + x2 = 16 * 10
            gt[b, TINY, :4] = [101, 101, 103, 103]                # grid centres are at 4 + 8 i: none inside
            gt[b, c - 2, :4] = [0, 0, hw[1] - 1, hw[0] - 1]
            gt[b, c - 1, :4] = gt[b, DUP, :4]
            gt[b, c - 1, 4] = (gt[b, DUP, 4] + 7) % NUM_CLASSES
    assert gt.astype(np.float32).astype(np.float64).tolist() == gt.tolist()       # the kernels see these values
    return gt, counts


def _oracle(gt, counts, hws, topk):
    """Per image: atss_assign's dict plus the oracle's (onehot, regression, state), or None without boxes."""
    _, a64, _, lv = _anchors()
    out = []
    for b in range(gt.shape[0]):
        ann = gt[b, :counts[b]]
        r = A.atss_assign(a64, lv, ann, topk) if counts[b] else {}
        r["onehot"], r["reg"], r["state"] = A.atss_targets_bbox(PAD_HW, ann, NUM_CLASSES, mask_shape=hws[b], topk=topk,
                                                                anchors=a64)
        out.append(r)
    return out


def _emulated_deviation(gt, counts, refs, topk):
    """The largest |fp32 - float64| of a candidate's IoU and of a threshold, the fp32 side computed on the CPU with
    the kernel's expressions."""
    a32, _, _, lv = _anchors()
    f = np.float32
    d_iou = d_thr = 0.0
    thr32 = A.atss_targets_torch(torch.from_numpy(a32), lv, torch.from_numpy(gt).float(), torch.tensor(counts),
                                 torch.tensor(HWS[:gt.shape[0]]), topk=topk, return_aux=True)[3].numpy()
    for b, r in enumerate(refs):
        if not counts[b]:
            continue
        an = a32[r["candidates"]]                                              # (n, N, 4)
        g = gt[b, :counts[b], None, :4].astype(f)
        iw = np.minimum(an[..., 2], g[..., 2]) - np.maximum(an[..., 0], g[..., 0]) + f(1)
        ih = np.minimum(an[..., 3], g[..., 3]) - np.maximum(an[..., 1], g[..., 1]) + f(1)
        inter = iw * ih
        ua = (an[..., 2] - an[..., 0] + f(1)) * (an[..., 3] - an[..., 1] + f(1)) \
            + (g[..., 2] - g[..., 0] + f(1)) * (g[..., 3] - g[..., 1] + f(1)) - inter
        iou = np.where((iw > 0) & (ih > 0), inter / ua, f(0))
        assert iou.dtype == np.float32
        d_iou = max(d_iou, float(np.abs(iou.astype(np.float64) - r["iou"]).max()))
        d_thr = max(d_thr, float(np.abs(thr32[b, :counts[b]].astype(np.float64) - r["threshold"]).max()))
    return d_iou, d_thr


def _excused(r, An, eps):
    """(near, tie): anchors with a qualifying candidacy within eps of its box's threshold; anchors whose two best
    qualifying IoUs lie within eps of each other without being equal."""
    near = np.zeros(An, dtype=bool)
    top1, top2 = np.full(An, -1.0), np.full(An, -1.0)
    for g in range(r["iou"].shape[0]):
        cand, iou, ins = r["candidates"][g], r["iou"][g], r["inside"][g]
        near[cand[ins & (np.abs(iou - r["threshold"][g]) <= eps)]] = True
        q = ins & (iou >= r["threshold"][g])
        c, v = cand[q], iou[q]
        top2[c] = np.where(v > top1[c], top1[c], np.maximum(top2[c], v))
        top1[c] = np.maximum(top1[c], v)
    tie = (top2 >= 0) & (top1 - top2 <= eps) & (top1 != top2)
    return near, tie


def _run(cuda, gt, counts, hws, topk):
    a32, _, c32, lv = _anchors()
    out = N.atss_targets(torch.from_numpy(a32).to(cuda), lv, torch.from_numpy(gt).float().to(cuda),
                         torch.tensor(counts, dtype=torch.int32, device=cuda),
                         torch.tensor(hws, dtype=torch.int32, device=cuda), topk=topk,
                         centers=torch.from_numpy(c32).to(cuda), return_aux=True)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _check(cuda, gt, counts, hws, topk, refs=None, eps=THR_EPS):
    """Run the kernels on the batch and compare every image with the float64 oracle; returns the outputs (numpy) and
    the oracle's per-image results."""
    a32, a64, c32, lv = _anchors()
    An, L = a32.shape[0], lv.shape[0]
    B, G = gt.shape[0], gt.shape[1]
    refs = refs or _oracle(gt, counts, hws, topk)
    state, label, reg, npos, thr, sel = [t.numpy() for t in _run(cuda, gt, counts, hws, topk)]
    assert state.shape == (B, An) and label.shape == (B, An) and reg.shape == (B, An, 4)
    assert thr.shape == (B, G) and sel.shape == (B, G, L, 16)
    reg = reg.astype(np.float64)
    assert npos.item() == int((state == 1).sum())
    for b in range(B):
        r, c = refs[b], counts[b]
        inside = ~((c32[:, 0] >= hws[b][1]) | (c32[:, 1] >= hws[b][0]))
        assert ((r["state"] == -1) == ~inside).all() and 0 < inside.sum()
        assert np.isin(state[b][inside], (0, 1)).all() and (state[b][~inside] == -1).all()
        assert np.isinf(thr[b, c:]).all() and (sel[b, c:] == -1).all()         # rows past the count: not read
        if c == 0:
            assert (state[b] == r["state"]).all() and (r["state"][inside] == 0).all()
            assert not label[b].any() and not reg[b].any()
            continue
        # pass 1: the selected locations exactly (in selection order), the threshold within THR_EPS
        assert (sel[b, :c, :, :topk] == r["selected"]).all() and (sel[b, :c, :, topk:] == -1).all()
        thr_err = np.abs(thr[b, :c].astype(np.float64) - r["threshold"])
        assert thr_err.max() <= eps, ("threshold", b, thr_err.argmax(), thr_err.max())
        margin = np.abs(r["iou"] - r["threshold"][:, None]).min()
        # pass 2
        near, tie = _excused(r, An, eps)
        pos = r["arg"] >= 0
        print("image {}: {} boxes, topk {}: {} positive, {} positive but outside, {} excused, {} unclear matches; "
              "worst threshold error {:.3e}, smallest |IoU - threshold| {:.3e}".format(
                  b, c, topk, int((r["state"] == 1).sum()), int((pos & ~inside).sum()), int(near.sum()),
                  int(tie.sum()), thr_err.max(), margin))
        assert near.sum() <= MAX_EXCUSED
        bad = ~near & (state[b] != r["state"])
        assert not bad.any(), ("state", b, np.nonzero(bad)[0][:8], state[b][bad][:8], r["state"][bad][:8])
        clear = ~near & ~tie
        assert clear.sum() > 0.95 * An
        r_label = np.where(pos, gt[b, np.maximum(r["arg"], 0), 4], 0).astype(np.int64)
        bad = clear & (label[b] != r_label)
        assert not bad.any(), ("label", b, np.nonzero(bad)[0][:8], label[b][bad][:8], r_label[bad][:8])
        on = clear & (r["state"] == 1)
        assert (r["onehot"][on].argmax(axis=1) == label[b][on]).all() and (r["onehot"][on].sum(axis=1) == 1).all()
        err = np.abs(reg[b] - r["reg"])
        bad = clear[:, None] & (err > REG_RTOL * np.maximum(1.0, np.abs(r["reg"])))
        assert not bad.any(), ("regression", b, np.nonzero(bad)[0][:8], reg[b][bad][:8], r["reg"][bad][:8])
        assert not reg[b][clear & ~pos].any() and not label[b][clear & ~pos].any()   # exactly 0 off the positives
    return (state, label, reg, npos, thr, sel), refs


@pytest.mark.parametrize("topk", [1, 9, 16])
@pytest.mark.parametrize("G", [12, 300])
def test_atss_against_the_oracle(cuda, G, topk):
    gt, counts = _batch(SEEDS[(G, topk)], G)
    refs = _oracle(gt, counts, HWS, topk)
    d_iou, d_thr = _emulated_deviation(gt, counts, refs, topk)
    margin = min(np.abs(r["iou"] - r["threshold"][:, None]).min() for r in refs if "iou" in r)
    print("G {} topk {}: emulated fp32 deviation from float64: IoU {:.3e}, threshold {:.3e}; THR_EPS {:.1e}; "
          "oracle margin {:.3e}".format(G, topk, d_iou, d_thr, THR_EPS, margin))
    assert 4 * max(d_iou, d_thr) <= THR_EPS
    assert margin >= MIN_MARGIN                                                # the seed: nothing is excused
    (state, label, _, _, thr, sel), _ = _check(cuda, gt, counts, HWS, topk, refs)
    _, a64, _, lv = _anchors()
    n_cand = sum(min(topk, h * w) for _, h, w, _ in lv.tolist()) * 9
    for b in (0, 2):
        r, c = refs[b], counts[b]
        assert r["candidates"].shape[1] == n_cand
        assert (state[b] == 1).sum() > 20 and (state[b] == 0).sum() > 5000
        # the anchor-shaped box holds its anchor; the tiny box holds nothing; the corner box's nearest locations
        assert r["best"][r["arg"] == ANCHOR_BOX].max() > 0.9
        assert not (r["arg"] == TINY).any()
        assert sel[b, CORNER, :, 0].tolist() == [30 * 40 + 37, 15 * 20 + 18, 7 * 10 + 9, 3 * 5 + 4, 1 * 3 + 2]
        # centre (80, 80): at strides 8 and 16 four locations tie for the nearest and the lowest index is taken; at
        # stride 32 it is a grid centre
        assert sel[b, BOUNDARY, :3, 0].tolist() == [9 * 40 + 9, 4 * 20 + 4, 2 * 10 + 2]
        # the duplicate in the last row loses every anchor to box DUP (in image 0 of G = 300 across the LDS tiles)
        m = r["arg"] == DUP
        assert m.sum() >= 1 and not (r["arg"] == c - 1).any() and (label[b][m] == int(gt[b, DUP, 4])).all()
        assert (sel[b, c - 1] == sel[b, DUP]).all() and thr[b, c - 1] == thr[b, DUP]
        # the whole-image box takes all six locations of the last level
        if topk >= 6:
            assert sorted(sel[b, c - 2, 4, :6].tolist()) == list(range(6)) and (sel[b, c - 2, 4, 6:] == -1).all()
    # anchors centred at or beyond (200, 300) are ignored in the smaller images, positives among them
    c32 = _anchors()[2]
    lost = (refs[2]["arg"] == CORNER) & ((c32[:, 0] >= 300) | (c32[:, 1] >= 200))
    assert lost.sum() >= 1 and (lost == (refs[2]["arg"] == CORNER)).all() and (state[2][lost] == -1).all()
    assert (state[0][refs[0]["arg"] == CORNER] == 1).all()
    assert (state[2] == -1).sum() > (state[0] == -1).sum() + 1000


def test_atss_two_calls_are_bitwise_equal(cuda):
    gt, counts = _batch(SEEDS[(300, 9)], 300)
    a, b = _run(cuda, gt, counts, HWS, 9), _run(cuda, gt, counts, HWS, 9)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[3].item() > 100


def test_atss_hip_against_the_fp32_torch_form(cuda):
    """Random boxes under a resize scale (non-integer fp32 corners): the distances are not exact any more, and the HIP
    selection must still equal the torch one bit for bit; the states agree off the excused band."""
    a32, a64, c32, lv = _anchors()
    An = a32.shape[0]
    G, topk = 300, 9
    gt, counts = _batch(SEEDS[(300, 9)], G)
    gt[..., :4] = (gt[..., :4].astype(np.float32) * np.float32(0.7371)).astype(np.float64)
    hws = [(188, 235), (147, 221), (147, 221)]
    dev = [torch.from_numpy(a32).to(cuda), lv, torch.from_numpy(gt).float().to(cuda),
           torch.tensor(counts, dtype=torch.int32, device=cuda), torch.tensor(hws, dtype=torch.int32, device=cuda)]
    centers = torch.from_numpy(c32).to(cuda)
    h = N.atss_targets(*dev, topk=topk, centers=centers, return_aux=True)
    t = A.atss_targets_torch(*dev, topk=topk, centers=centers, return_aux=True)
    torch.cuda.synchronize()
    assert torch.equal(h[5][..., :topk], t[4]) and bool((h[5][..., topk:] == -1).all())
    thr_h, thr_t = h[4].cpu().numpy(), t[3].cpu().numpy()
    for b, c in enumerate(counts):
        assert np.isinf(thr_h[b, c:]).all() and np.isinf(thr_t[b, c:]).all()
        if not c:
            assert torch.equal(h[0][b], t[0][b])
            continue
        assert np.abs(thr_h[b, :c] - thr_t[b, :c]).max() <= THR_EPS
        near, _ = _excused(A.atss_assign(a64, lv, gt[b, :c], topk), An, THR_EPS)
        differ = (h[0][b] != t[0][b]).cpu().numpy()
        print("image {}: {} excused, {} states differ, threshold difference {:.3e}".format(
            b, int(near.sum()), int(differ.sum()), np.abs(thr_h[b, :c] - thr_t[b, :c]).max()))
        assert near.sum() <= MAX_EXCUSED and not (differ & ~near).any()
    assert h[3].item() == int((h[0] == 1).sum()) > 100


def test_atss_refusals(cuda):
    a32, _, c32, lv = _anchors()
    gt, counts = _batch(SEEDS[(12, 9)], 12)
    args = [torch.from_numpy(a32).to(cuda), lv, torch.from_numpy(gt).float().to(cuda),
            torch.tensor(counts, dtype=torch.int32, device=cuda), torch.tensor(HWS, dtype=torch.int32, device=cuda)]
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="topk"):
            N.atss_targets(*args, topk=k)
    short = lv.copy()
    short[-1, 1] = 1                                    # 2 x 3 -> 1 x 3: 27 anchors missing
    with pytest.raises(ValueError, match="add up"):
        N.atss_targets(args[0], short, *args[2:])
    shifted = lv.copy()
    shifted[1, 0] += 9
    with pytest.raises(ValueError, match="add up"):
        N.atss_targets(args[0], shifted, *args[2:])
    with pytest.raises(ValueError, match="add up"):
        N.atss_targets(args[0][:-1], lv, *args[2:])
    # the library's own check (the Python one bypassed): an error code, no launch
    table = (N.c_int * 20)(*[int(v) for v in shifted.reshape(-1)])
    assert N.lib().mxr_atss_targets(None, None, 15354, table, 5, None, 1, 1, None, None, 9, None, None, None, None,
                                    None, None, None, 0.2, None) != 0
    assert N.lib().mxr_atss_targets(None, None, 15354, table, 5, None, 1, 1, None, None, 17, None, None, None, None,
                                    None, None, None, 0.2, None) != 0
