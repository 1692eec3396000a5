"""The IoU regression loss kernel (``iou_loss_kernel<T, KIND>`` of csrc/kernels/losses.hip, through
``native.iou_loss_fwd_bwd``) per element against float64: the float64 autograd of the formula as restated below
(independently of ops/losses.py), on the values the kernel receives (predictions rounded to its input type first).

Inputs: the 2,907 anchors of a 96 x 160 image, two images of 12 boxes each with sides of 12 .. 82 px, state and
regression target from ``anchor_targets_torch``, prediction = target + noise * randn.  Noise 1 gives overlapping
boxes, noise 6 flipped and disjoint ones (at least 50 of each, asserted).

A selection (corner order, prediction's corner against the target's, overlap against 0) may legitimately fall the
other way in fp32 than in float64: a positive row in which one of the eight differences is below 1e-4 of the
anchor's side is left out of the gradient comparison; at most 2 % of the positive rows may be, asserted before the
kernel's output is looked at.

Metric: the four gradient elements of a row cancel, so the bound is on the row's scale g_r = max_j |ref[r, j]|:
    fp32   |got - ref| <= RTOL32 * g_r
    bf16   |got - ref| <= 2^-8 |ref| + RTOL32 * g_r        (one rounding to bf16 with the margin of the smooth-L1 test)
RTOL32: PyTorch's own fp32 autograd (on the CPU) of the same formula (``_formula`` below, in fp32) on this file's
inputs, seeds 0 and 1, against the float64 reference under this metric needs
    noise 1:  giou 3.68e-7 .. 4.25e-7   diou 5.64e-7 .. 6.75e-7   ciou 5.10e-7 .. 6.75e-7
    noise 6:  giou 1.13e-6 .. 2.30e-6   diou 7.12e-7 .. 1.41e-6   ciou 1.42e-6 .. 2.30e-6
(the ranges over fp32 / bf16-rounded predictions and the two seeds; 435 / 570 positives, at noise 6 206 / 270 of
them flipped and 161 / 193 disjoint, none within 1e-4 of a tie): 2.30e-6 at worst.  The kernel gets 8x that,
1.84e-5, the margin test_losses_gpu.py gives the focal kernel and for its reason: the kernel's divisions and atan
are good to an ulp or two, not correctly rounded.  The loss agrees with float64 to 1e-5 relative.
"""
import functools
import math

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops.anchors import anchor_targets_torch, anchors_for_shape

pytestmark = pytest.mark.gpu

KINDS = ["giou", "diou", "ciou"]
DTYPES = [torch.float32, torch.bfloat16]
S = 0.2                 # BOX_STD
EPS = 1e-7
TIE = 1e-4              # of the anchor's side
MAX_LEFT_OUT = 0.02
RTOL32_TORCH = 2.30e-6
RTOL32 = 8 * RTOL32_TORCH
RTOL_BF16 = 2.0 ** -8
LOSS_RTOL = 1e-5
GROUP, LD = 9, 64       # the packed regression final's padded rows


# ------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------
def _boxes(an, d):
    aw, ah = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    return (an[:, 0] + S * d[:, 0] * aw, an[:, 1] + S * d[:, 1] * ah, an[:, 2] + S * d[:, 2] * aw,
            an[:, 3] + S * d[:, 3] * ah)


def _formula(an, pred, target, kind):
    """Per-row loss in the dtype of the arguments ((N, 4) each), for autograd; and the eight differences the
    selections look at, relative to the anchor's side."""
    aw, ah = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    gx1, gy1, gx2, gy2 = _boxes(an, target)
    qx1, qy1, qx2, qy2 = _boxes(an, pred)
    px1, px2 = torch.minimum(qx1, qx2), torch.maximum(qx1, qx2)
    py1, py2 = torch.minimum(qy1, qy2), torch.maximum(qy1, qy2)
    iwr = torch.minimum(px2, gx2) - torch.maximum(px1, gx1)
    ihr = torch.minimum(py2, gy2) - torch.maximum(py1, gy1)
    inter = iwr.clamp_min(0) * ihr.clamp_min(0)
    union = (px2 - px1) * (py2 - py1) + (gx2 - gx1) * (gy2 - gy1) - inter + EPS
    iou = inter / union
    cw = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    ch = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    if kind == "giou":
        c = cw * ch + EPS
        loss = 1 - iou + (c - union) / c
    else:
        c2 = cw ** 2 + ch ** 2 + EPS
        rho2 = ((px1 + px2 - gx1 - gx2) ** 2 + (py1 + py2 - gy1 - gy2) ** 2) / 4
        loss = 1 - iou + rho2 / c2
        if kind == "ciou":
            v = 4 / math.pi ** 2 * (torch.atan((gx2 - gx1) / (gy2 - gy1 + EPS))
                                    - torch.atan((px2 - px1) / (py2 - py1 + EPS))) ** 2
            alpha = (v / (1 - iou + v + EPS)).detach()
            loss = loss + alpha * v
    sel = torch.stack([(qx1 - qx2) / aw, (qy1 - qy2) / ah, (px1 - gx1) / aw, (px2 - gx2) / aw, (py1 - gy1) / ah,
                       (py2 - gy2) / ah, iwr / aw, ihr / ah], 1).detach()
    return loss, sel


def iou_ref(pred, target, anchors, state, npos, kind, weight=1.0, dtype=torch.float64):
    """loss (python float), gradient [R, 4] and per row: compared (positive, away from every tie), flipped, disjoint.
    ``dtype=torch.float32`` is the fp32 autograd yardstick of RTOL32."""
    R, A = pred.shape[0], anchors.shape[0]
    pos = (state == 1).nonzero().flatten()
    p = pred[pos].to(dtype).requires_grad_(True)
    rows, sel = _formula(anchors[pos % A].to(dtype), p, target[pos].to(dtype), kind)
    total = weight * rows.sum() / max(1, int(npos))
    grad = torch.zeros(R, 4, dtype=dtype, device=pred.device)
    if pos.numel():
        total.backward()
        grad[pos] = p.grad
    masks = []
    for m in ((sel.abs() >= TIE).all(1), (sel[:, :2] > 0).any(1), (sel[:, 6:] < 0).any(1)):
        full = torch.zeros(R, dtype=torch.bool, device=pred.device)
        full[pos] = m
        masks.append(full)
    return total.item(), grad, masks[0], masks[1], masks[2]


def grad_need(got, ref, compared, rel=0.0):
    """The RTOL32 the compared rows need: max over their elements of (|got - ref| - rel |ref|) / g_r."""
    ref = ref[compared]
    err = (got.double()[compared] - ref).abs() - rel * ref.abs()
    scale = ref.abs().max(1, keepdim=True).values
    assert bool((scale > 0).all())
    return (err / scale).max().clamp_min(0).item() if ref.numel() else 0.0


# ------------------------------------------------------------------------------------------------
# inputs (generated on the host: the same bits whatever the device)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _targets(shape, B, seed):
    H, W = shape
    gen = torch.Generator().manual_seed(seed)
    anchors = torch.from_numpy(anchors_for_shape((H, W, 3)).astype(np.float32))
    G = 12
    wh = 12 + 70 * torch.rand(B, G, 2, generator=gen)
    xy = torch.rand(B, G, 2, generator=gen) * (torch.tensor([W, H], dtype=torch.float32) - wh)
    gt = torch.cat([xy, xy + wh, torch.randint(0, 8, (B, G, 1), generator=gen).float()], 2)
    state, _, target = anchor_targets_torch(anchors, gt, torch.full((B,), G), torch.tensor([[H, W]] * B))
    return anchors, state.reshape(-1).contiguous(), target.reshape(-1, 4).contiguous()


@functools.lru_cache(maxsize=None)
def iou_inputs(noise, dtype, seed=0, shape=(96, 160), B=2):
    """anchors [A, 4] f32, pred [B A, 4] dtype, target [B A, 4] f32, state [B A] int8 (on the host)."""
    anchors, state, target = _targets(shape, B, seed)
    gen = torch.Generator().manual_seed(1000 + seed)
    pred = (target + noise * torch.randn(target.shape, generator=gen)).to(dtype)
    return anchors, pred, target, state


def _check_loss(got, ref, what):
    got = float(got)
    print("{}: loss {!r} ref {!r} rel {:.3e}".format(what, got, ref, abs(got - ref) / abs(ref) if ref else 0.0))
    assert math.isfinite(got), what
    assert abs(got - ref) <= LOSS_RTOL * abs(ref), (what, got, ref)


def _check_grad(got, ref, compared, state, dtype, what):
    rel = RTOL_BF16 if dtype == torch.bfloat16 else 0.0
    need = grad_need(got, ref, compared, rel)
    print("{}: worst RTOL32 needed {:.3e} (allowed {:.3e}) over {} rows".format(what, need, RTOL32,
                                                                               int(compared.sum())))
    assert not got[state != 1].any(), what + ": a row that is not positive has a gradient"
    assert bool(torch.isfinite(got.float()).all()), what
    assert need <= RTOL32, (what, need)


def _run(cuda, kind, dtype, noise, npos=None, weight=1.0, seed=0, shape=(96, 160), B=2, counts=False):
    anchors, pred, target, state = (t.to(cuda) for t in iou_inputs(noise, dtype, seed, shape, B))
    R, A = pred.shape[0], anchors.shape[0]
    assert R % GROUP == 0 and R == B * A
    n = int((state == 1).sum().item()) if npos is None else npos
    npos_t = None if npos is None else torch.tensor([npos], dtype=torch.int32, device=cuda)
    ref_loss, ref_grad, compared, flipped, disjoint = iou_ref(pred, target, anchors, state, n, kind, weight)
    P = int((state == 1).sum().item())
    left_out = P - int(compared.sum().item())
    what = "{} {} noise={} rows={}".format(kind, str(dtype)[6:], noise, R)
    print("{}: {} positives, {} flipped, {} disjoint, {} left out near a tie".format(
        what, P, int(flipped.sum()), int(disjoint.sum()), left_out))
    assert P >= 100 and left_out <= MAX_LEFT_OUT * P
    if counts:
        assert int(flipped.sum()) >= 50 and int(disjoint.sum()) >= 50
    loss, grad = N.iou_loss_fwd_bwd(pred, target, anchors, state, npos=npos_t, kind=kind, weight=weight)
    assert grad.dtype == dtype and grad.shape == pred.shape
    _check_grad(grad, ref_grad, compared, state, dtype, what)
    _check_loss(loss, ref_loss, what)
    # the padded layout: the same bits, the padding columns untouched
    buf = torch.zeros(R // GROUP, LD, dtype=dtype, device=cuda)
    loss2, g2 = N.iou_loss_fwd_bwd(pred, target, anchors, state, npos=npos_t, kind=kind, weight=weight, grad_out=buf,
                                   group=GROUP)
    assert g2 is buf
    assert not buf[:, GROUP * 4:].any(), "padding columns written"
    assert torch.equal(loss2, loss) and torch.equal(buf[:, :GROUP * 4].reshape(R, 4), grad)
    return loss, grad


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [1.0, 6.0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_iou_loss_forms(cuda, dtype, kind, noise):
    _run(cuda, kind, dtype, noise, counts=noise == 6.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_iou_loss_explicit_npos(cuda, dtype, kind):
    """The kernel divides by the npos it is handed, not by the positive rows it sees."""
    _run(cuda, kind, dtype, 6.0, npos=57)


@pytest.mark.parametrize("kind", KINDS)
def test_iou_loss_weight(cuda, kind):
    """weight = 2 against float64, and bit for bit twice the weight = 1 result in fp32."""
    l1, g1 = _run(cuda, kind, torch.float32, 6.0)
    l2, g2 = _run(cuda, kind, torch.float32, 6.0, weight=2.0)
    assert torch.equal(l2, 2 * l1) and torch.equal(g2, 2 * g1)
    _run(cuda, kind, torch.bfloat16, 6.0, weight=2.0)


@pytest.mark.parametrize("fill", [0, -1], ids=["no_positives", "all_ignored"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_iou_loss_nothing_to_learn(cuda, dtype, kind, fill):
    anchors, pred, target, state = (t.to(cuda) for t in iou_inputs(6.0, dtype))
    state = torch.full_like(state, fill)
    R = pred.shape[0]
    loss, grad = N.iou_loss_fwd_bwd(pred, target, anchors, state, kind=kind)
    buf = torch.zeros(R // GROUP, LD, dtype=dtype, device=cuda)
    loss2, _ = N.iou_loss_fwd_bwd(pred, target, anchors, state, kind=kind, grad_out=buf, group=GROUP)
    assert loss.item() == 0.0 and loss2.item() == 0.0
    assert not grad.any() and not buf.any()


def test_iou_loss_second_grid_trip(cuda):
    """6 x 91,260 anchors of a 608 x 800 image = 547,560 rows > 2048 x 256 threads (and a multiple of 9): the
    grid-stride loop takes a second trip."""
    anchors = iou_inputs(6.0, torch.bfloat16, 0, (608, 800), 6)[0]
    assert anchors.shape[0] == 91260 and 6 * 91260 > N.LOSS_GRID * 256
    _run(cuda, "giou", torch.bfloat16, 6.0, shape=(608, 800), B=6)


def test_iou_loss_argument_checks(cuda):
    """A bad layout is refused before any launch: by the wrapper, and by the entry point itself (-1)."""
    anchors, pred, target, state = (t.to(cuda) for t in iou_inputs(1.0, torch.bfloat16))
    R = pred.shape[0]
    with pytest.raises(ValueError):
        N.iou_loss_fwd_bwd(pred, target, anchors, state, kind="iou")
    with pytest.raises(ValueError):
        N.iou_loss_fwd_bwd(pred, target, anchors[:-1], state)                      # rows % A != 0
    with pytest.raises(ValueError):
        N.iou_loss_fwd_bwd(pred, target, anchors.double(), state)
    with pytest.raises(ValueError):
        N.iou_loss_fwd_bwd(pred, target[:-1], anchors, state)
    with pytest.raises(ValueError):                                                # fp32 grad_out for bf16 deltas
        N.iou_loss_fwd_bwd(pred, target, anchors, state, grad_out=torch.zeros(R // 9, 64, device=cuda), group=9)
    with pytest.raises(RuntimeError):                                              # 4 * group > ld
        N.iou_loss_fwd_bwd(pred, target, anchors, state, group=9,
                           grad_out=torch.zeros(R // 9, 32, dtype=torch.bfloat16, device=cuda))
    part = torch.empty(N.LOSS_GRID, device=cuda)
    out = torch.empty(1, device=cuda)
    npos = torch.ones(1, dtype=torch.int32, device=cuda)
    grad = torch.zeros_like(pred)

    def entry(rows, A, kind, grp=0, ld=0):
        return N.lib().mxr_iou_loss_fwd_bwd(pred.data_ptr(), target.data_ptr(), anchors.data_ptr(), state.data_ptr(),
                                            npos.data_ptr(), grad.data_ptr(), part.data_ptr(), out.data_ptr(), rows, A,
                                            kind, 1.0, 1, grp, ld, torch.cuda.current_stream().cuda_stream)

    A = anchors.shape[0]
    assert entry(R, A, 3) == -1 and entry(R, A, -1) == -1                          # unknown kind
    assert entry(R, A - 1, 0) == -1 and entry(R, 0, 0) == -1                       # rows % A != 0, no anchors
    assert entry(R, A, 0, 9, 32) == -1 and entry(R, A, 0, 0, 64) == -1 and entry(R, A, 0, 7, 64) == -1
    torch.cuda.synchronize()
    assert not grad.any()                                                          # nothing ran
    assert entry(R, A, 0) == 0                                                     # the accepted form of the call
    torch.cuda.synchronize()
    assert grad.any()
