"""Task-aligned assignment on the CPU: the float64 oracle of ``ops/anchors.py`` (``tal_assign``) against a hand-written
triple loop and on hand-made cases (the tie rules, empty boxes, K above the candidate count, the quality's
normalisation), the fp32 torch form against it, and ``quality_loss(..., quality=q)``.

Hand-made cases: a 64 x 64 image, levels 8x8, 4x4, 2x2, 1x1 and 1x1 (strides 8..128), 774 anchors."""
import math

import numpy as np
import pytest
import torch

import tal_common as TC
from batchai_retinanet_horovod_coco_amd.ops import anchors as A
from batchai_retinanet_horovod_coco_amd.ops import losses as L

PAD = (64, 64)
C = 5
ANCHORS = A.anchors_for_shape(PAD)
LEVELS = A.level_table(PAD)
GRID = [(8, 8, 8), (4, 4, 16), (2, 2, 32), (1, 1, 64), (1, 1, 128)]
NA = ANCHORS.shape[0]


def _ann(*rows):
    return np.asarray(rows, dtype=np.float64).reshape(-1, 5)


def _preds(seed, scale=0.5):
    rng = np.random.RandomState(seed)
    return rng.randn(NA, C) * 2 - 2, rng.randn(NA, 4) * scale


# ------------------------------------------------------------------------------------------------ the oracle by hand
def _by_hand(boxes, x, d, topk):
    """The rule with plain loops: (arg per anchor, quality per anchor, selected sets per box)."""
    centre = []
    for h, w, s in GRID:
        centre += [((loc % w + 0.5) * s, (loc // w + 0.5) * s) for loc in range(h * w) for _ in range(9)]
    n = len(boxes)
    u = [[0.0] * NA for _ in range(n)]
    t = [[0.0] * NA for _ in range(n)]
    selected = []
    for j, (x1, y1, x2, y2, lab) in enumerate(boxes):
        cand = []
        for i in range(NA):
            a = ANCHORS[i]
            aw, ah = a[2] - a[0], a[3] - a[1]
            q = [a[0] + d[i][0] * 0.2 * aw, a[1] + d[i][1] * 0.2 * ah, a[2] + d[i][2] * 0.2 * aw, a[3] + d[i][3] * 0.2 * ah]
            px1, px2, py1, py2 = min(q[0], q[2]), max(q[0], q[2]), min(q[1], q[3]), max(q[1], q[3])
            iw, ih = max(min(px2, x2) - max(px1, x1), 0.0), max(min(py2, y2) - max(py1, y1), 0.0)
            inter = iw * ih
            u[j][i] = inter / ((px2 - px1) * (py2 - py1) + (x2 - x1) * (y2 - y1) - inter + 1e-7)
            s = 1.0 / (1.0 + math.exp(-x[i][int(lab)]))
            t[j][i] = s * u[j][i] * u[j][i] * u[j][i] * u[j][i] * u[j][i] * u[j][i]
            cx, cy = centre[i]
            if min(cx - x1, cy - y1, x2 - cx, y2 - cy) > 0.01 and u[j][i] > 0:
                cand.append(i)
        cand.sort(key=lambda i: (-t[j][i], i))
        selected.append(cand[:topk])
    arg = [-1] * NA
    for i in range(NA):
        for j in range(n):
            if i in selected[j] and (arg[i] < 0 or u[j][i] > u[arg[i]][i]):
                arg[i] = j
    quality = [0.0] * NA
    for j in range(n):
        held = [i for i in range(NA) if arg[i] == j]
        if held:
            tmax, umax = max(t[j][i] for i in held), max(u[j][i] for i in held)
            for i in held:
                quality[i] = t[j][i] / (tmax + 1e-7) * umax
    return arg, quality, selected


def test_tal_assign_against_a_triple_loop():
    boxes = _ann([4, 6, 40, 50, 1], [20, 10, 60, 44, 3], [0, 0, 63, 63, 0], [30, 30, 47, 52, 4], [8, 28, 30, 60, 2])
    x, d = _preds(3)
    for topk in (1, 13):
        r = A.tal_assign(ANCHORS, LEVELS, boxes, x, d, topk)
        arg, quality, selected = _by_hand(boxes.tolist(), x.tolist(), d.tolist(), topk)
        assert r["arg"].tolist() == arg
        for j in range(5):
            assert sorted(np.nonzero(r["selected"][j])[0].tolist()) == sorted(selected[j])
        # (the sixth power is u2 * u2 * u2 in the oracle and a chain here: a few ulps)
        assert np.allclose(r["quality"], quality, rtol=1e-12, atol=0)
        assert (np.asarray(arg) >= 0).sum() >= 5 * topk * 0.6 and len(set(arg)) > 3


def test_equal_metrics_go_to_the_lower_anchor_index():
    """Nine identical anchors per location with identical predictions: equal t in any precision."""
    same = ANCHORS.reshape(-1, 9, 4)[:, 4:5].repeat(9, axis=1).reshape(-1, 4)
    x, d = np.zeros((NA, C)), np.zeros((NA, 4))
    r = A.tal_assign(same, LEVELS, _ann([10, 10, 30, 30, 2]), x, d, topk=1)
    (sel,) = np.nonzero(r["selected"][0])
    assert len(sel) == 1 and sel[0] % 9 == 0
    assert (r["t"][0, sel[0]:sel[0] + 9] == r["t"][0, sel[0]]).all()
    r = A.tal_assign(same, LEVELS, _ann([10, 10, 30, 30, 2]), x, d, topk=4)
    (sel4,) = np.nonzero(r["selected"][0])
    assert sel4.tolist() == list(range(sel[0], sel[0] + 4))
    # a logit so negative that every score is 0: every t is 0, and the first candidates are taken
    r = A.tal_assign(ANCHORS, LEVELS, _ann([10, 10, 30, 30, 2]), np.full((NA, C), -1e4), d, topk=5)
    cand = np.nonzero(r["candidate"][0])[0]
    assert not r["t"][0].any() and np.nonzero(r["selected"][0])[0].tolist() == cand[:5].tolist()


def test_a_duplicated_box_loses_every_anchor_to_the_first():
    x, d = _preds(4)
    boxes = _ann([4, 6, 40, 50, 1], [20, 10, 60, 44, 3], [4, 6, 40, 50, 2])
    r = A.tal_assign(ANCHORS, LEVELS, boxes, x, d, topk=13)
    # with the same logit column the two would select the same anchors; under another label they select their own,
    # and an anchor both selected stays with box 0
    both = r["selected"][0] & r["selected"][2]
    assert (r["arg"] == 0).sum() >= 1 and not (r["arg"][both] == 2).any()
    boxes[2, 4] = 1
    r = A.tal_assign(ANCHORS, LEVELS, boxes, x, d, topk=13)
    assert (r["selected"][0] == r["selected"][2]).all() and (r["arg"] == 0).sum() >= 1 and not (r["arg"] == 2).any()
    assert r["tmax"][2] == 0 and r["umax"][2] == 0


def test_boxes_that_get_nothing():
    x, d = _preds(5)
    # grid centres are at 4 + 8 i: none inside [33, 35]
    r = A.tal_assign(ANCHORS, LEVELS, _ann([33, 33, 35, 35, 1], [4, 6, 40, 50, 1]), x, d, topk=13)
    assert r["count"][0] == 0 and not r["selected"][0].any() and not (r["arg"] == 0).any()
    assert np.isnan(r["cutoff"][0]).all() and (r["arg"] == 1).sum() == 13
    # every predicted box far away from the image: u = 0 for all, centre inside or not
    r = A.tal_assign(ANCHORS, LEVELS, _ann([4, 6, 40, 50, 1]), x, np.full((NA, 4), 1000.0), topk=13)
    assert not r["u"].any() and r["count"][0] == 0 and (r["arg"] == -1).all() and not r["quality"].any()
    labels, reg, state, q = A.tal_targets_bbox(PAD, _ann([4, 6, 40, 50, 1]), x, np.full((NA, 4), 1000.0), anchors=ANCHORS)
    # (the two coarsest levels' single location is centred at (64, 64): outside, state -1)
    assert not (state == 1).any() and (state == 0).sum() > 700 and not labels[state == 0].any() and not reg.any() \
        and not q.any()
    labels, reg, state, q = A.tal_targets_bbox(PAD, _ann(), x, d, anchors=ANCHORS)
    # (the two coarsest levels' single location is centred at (64, 64): outside, state -1)
    assert not (state == 1).any() and (state == 0).sum() > 700 and not labels[state == 0].any() and not reg.any() \
        and not q.any()


def test_topk_above_the_candidate_count_takes_all():
    x = _preds(6)[0]
    r = A.tal_assign(ANCHORS, LEVELS, _ann([2, 2, 6, 6, 0]), x, np.zeros((NA, 4)), topk=13)     # centre (4, 4) alone
    assert r["count"][0] == 9 and np.nonzero(r["selected"][0])[0].tolist() == list(range(9))
    assert (r["arg"][:9] == 0).all() and (r["arg"][9:] == -1).all() and np.isnan(r["cutoff"][0, 1])
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="topk"):
            A.tal_assign(ANCHORS, LEVELS, _ann([2, 2, 6, 6, 0]), x, np.zeros((NA, 4)), topk=k)


def test_the_best_anchor_of_a_box_gets_its_largest_iou_as_quality():
    # max q = tmax / (tmax + 1e-7) * umax: the 1e-7 costs umax * 1e-7 / tmax, below 1e-6 from tmax = 0.1 umax on --
    # boxes an anchor fits (rounded anchors) and predictions of a model that has begun to fit (scores near 0.9, boxes
    # within a tenth of the anchor's size)
    fit = np.nonzero((ANCHORS[:, :2] >= 0).all(axis=1) & (ANCHORS[:, 2:] <= 63).all(axis=1))[0]
    boxes = np.concatenate([np.round(ANCHORS[fit[np.linspace(0, len(fit) - 1, 5).astype(int)]]),
                            np.asarray([[1], [3], [0], [4], [2]], dtype=np.float64)], axis=1)
    for seed in (7, 8):
        x, d = _preds(seed, scale=0.1)
        x = x + 4
        r = A.tal_assign(ANCHORS, LEVELS, boxes, x, d, topk=13)
        seen = 0
        for j in range(5):
            held = r["arg"] == j
            if held.any():
                seen += 1
                assert r["tmax"][j] >= 0.1 * r["umax"][j]
                assert abs(r["quality"][held].max() - r["umax"][j]) <= 1e-6
                assert (r["quality"][held] > 0).all() and (r["quality"][held] <= r["umax"][j]).all()
        assert seen >= 4 and not r["quality"][r["arg"] < 0].any()
    labels, reg, state, q = A.tal_targets_bbox(PAD, boxes, x, d, mask_shape=(40, 64), anchors=ANCHORS)
    outside = (ANCHORS[:, 1] + ANCHORS[:, 3]) / 2 >= 40
    assert (state[outside] == -1).all() and (labels[outside] == -1).all() and not q[outside].any()
    assert ((r["arg"] >= 0) & outside).any()                # positives among the ignored: the rule is applied last
    on = state == 1
    assert (labels[on].sum(axis=1) == 1).all() and (labels[on].argmax(axis=1) == boxes[r["arg"][on], 4]).all()
    assert np.allclose(reg[on], A.bbox_transform(ANCHORS[on], boxes[r["arg"][on], :4])) and not reg[state == 0].any()


# ------------------------------------------------------------------------------------------------ the torch form
# EPS32, the relative band of the metric t inside which an fp32 form may order two candidates either way (and of u, for
# two boxes that selected one anchor): the fp32 expressions emulated in numpy (tal_common.emulate32) differ from
# float64 by at most 1.511e-5 relative in t over the candidates whose t is at least half their box's cut-off (G = 300,
# topk 13, trained; 5.8e-6 .. 6.7e-6 in the other cases: image coordinates cost the fp32 intersection digits, and the
# sixth power multiplies u's error by six); 4 x that, rounded up.  QTOL: the quality emulated the same way on the
# oracle's assignment is off by at most 6.049e-6; 4 x that, rounded up.  The test recomputes both maxima and refuses
# larger ones; the seeds leave no candidacy of the float64 oracle inside the band, so no anchor is excused (asserted).
EPS32 = 6.2e-5
QTOL = 2.5e-5
TORCH_SEEDS = {("trained", 12): 100, ("untrained", 12): 100, ("trained", 300): 100, ("untrained", 300): 105}


@pytest.mark.parametrize("G", [12, 300])
@pytest.mark.parametrize("kind", ["trained", "untrained"])
def test_torch_form_against_the_oracle(kind, G):
    a32, a64, c32, lv = TC.anchors()
    topk, seed = 13, TORCH_SEEDS[(kind, G)]
    gt, counts = TC.batch(seed, G)
    logits, deltas = TC.predictions(seed, 3, kind)
    refs = TC.oracle(gt, counts, TC.HWS, logits, deltas, topk)
    d_t, d_q = TC.emulated_deviation(gt, counts, refs, logits, deltas)
    print("{} G {}: emulated fp32 deviation from float64: t {:.3e} relative, quality {:.3e}".format(kind, G, d_t, d_q))
    assert 4 * d_t <= EPS32 and 4 * d_q <= QTOL
    state, label, reg, q = A.tal_targets_torch(torch.from_numpy(a32), lv, torch.from_numpy(gt).float(),
                                                torch.tensor(counts), torch.tensor(TC.HWS), logits, deltas, topk=topk,
                                                centers=torch.from_numpy(c32))
    assert state.dtype == torch.int8 and label.dtype == torch.int32 and reg.dtype == q.dtype == torch.float32
    state, label, reg, q = state.numpy(), label.numpy(), reg.numpy().astype(np.float64), q.numpy().astype(np.float64)
    for b, r in enumerate(refs):
        if not counts[b]:
            assert (state[b] == r["state"]).all() and not label[b].any() and not reg[b].any() and not q[b].any()
            continue
        near, tie = TC.excused(r, EPS32)
        assert near.sum() == 0                                  # the seed: nothing is excused
        assert (state[b] == r["state"]).all()
        clear = ~tie
        assert clear.sum() > 0.95 * clear.size
        pos = r["arg"] >= 0
        assert (label[b][clear] == np.where(pos, gt[b, np.maximum(r["arg"], 0), 4], 0)[clear]).all()
        err = np.abs(reg[b] - r["reg"])
        assert not (clear[:, None] & (err > 1e-5 * np.maximum(1.0, np.abs(r["reg"])))).any()
        # quality: the rows of boxes none of whose anchors is an unclear match (tmax and umax are the box's)
        qrows = clear & ~np.isin(r["arg"], np.unique(r["arg"][tie & pos]))
        assert np.abs(q[b] - r["q"])[qrows].max() <= QTOL
        assert (qrows & (r["state"] == 1)).sum() >= 0.9 * (r["state"] == 1).sum()
        assert (state[b] == 1).sum() > 20 and not q[b][state[b] != 1].any()
        if G == 300:
            assert (r["selected"].sum(axis=0) > 1).sum() > 100  # contested anchors: the conflict rule is exercised


def test_torch_form_without_box_slots():
    a32, _, c32, lv = TC.anchors()
    logits, deltas = TC.predictions(1, 2, "trained", torch.float32)
    state, label, reg, q = A.tal_targets_torch(torch.from_numpy(a32), lv, torch.zeros(2, 0, 5), torch.zeros(2).int(),
                                                torch.tensor([[256, 320], [200, 300]]), logits, deltas,
                                                centers=torch.from_numpy(c32))
    assert not (state == 1).any() and (state[1] == -1).sum() > (state[0] == -1).sum() + 1000
    assert not label.any() and not reg.any() and not q.any()
    with pytest.raises(ValueError, match="logits"):
        A.tal_targets_torch(torch.from_numpy(a32), lv, torch.zeros(2, 0, 5), torch.zeros(2).int(),
                            torch.tensor([[256, 320], [200, 300]]), logits[:, :-1], deltas)


# ------------------------------------------------------------------------------------------------ quality_loss(quality=)
def _quality_loop(x, state, label, q, kind):
    total = 0.0
    for r in range(x.shape[0]):
        if state[r] == -1:
            continue
        for c in range(x.shape[1]):
            v = float(x[r, c])
            sp = max(v, 0.0) + math.log1p(math.exp(-abs(v)))
            p = 1.0 / (1.0 + math.exp(-v))
            t = float(q[r]) if (state[r] == 1 and label[r] == c) else 0.0
            if kind == "qfl":
                total += (p - t) ** 2 * (sp - t * v)
            else:
                total += t * (sp - t * v) if t > 0 else 0.75 * p * p * sp
    return total / max(1, int((state == 1).sum()))


@pytest.mark.parametrize("kind", ["qfl", "vfl"])
def test_quality_loss_with_a_given_target(kind):
    g = torch.Generator().manual_seed(11)
    B, An, Cn = 2, 40, 6
    x = (torch.randn(B, An, Cn, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    state = torch.randint(-1, 2, (B, An), generator=g).to(torch.int8)
    label = torch.randint(0, Cn, (B, An), generator=g).to(torch.int32)
    q = torch.rand(B, An, generator=g, dtype=torch.float64)
    q[0, :3] = 0                                            # a positive row may have quality 0 (VFL's other branch)
    loss = L.quality_loss(x, None, None, state, label, None, kind, backend="torch", quality=q)
    ref = _quality_loop(x.detach().reshape(-1, Cn).numpy(), state.reshape(-1).numpy(), label.reshape(-1).numpy(),
                        q.reshape(-1).numpy(), kind)
    assert abs(float(loss.detach()) - ref) <= 1e-12 * abs(ref)
    assert torch.autograd.gradcheck(
        lambda v: L.quality_loss(v, None, None, state, label, None, kind, backend="torch", quality=q), (x,))
    # the quality of rows that are not positive is not read
    q2 = torch.where(state == 1, q, torch.full_like(q, 7.0))
    assert float(L.quality_loss(x, None, None, state, label, None, kind, backend="torch", quality=q2)) == float(loss)
    # and it is the existing expression when q is that expression's own IoU
    an = torch.tensor([[0.0, 0, 10, 10]] * An, dtype=torch.float64)
    reg, reg_t = torch.randn(B, An, 4, generator=g, dtype=torch.float64), torch.randn(B, An, 4, generator=g) * 0.5
    own = L.quality_targets(an, reg, reg_t, state)
    assert float(L.quality_loss(x, reg, reg_t, state, label, an, kind, backend="torch")) == \
        float(L.quality_loss(x, None, None, state, label, None, kind, backend="torch", quality=own))
    # no kernel reads a given target: asking for one is an error, not a quiet torch expression
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        L.quality_loss(x, None, None, state, label, None, kind, backend="hip", quality=q)
