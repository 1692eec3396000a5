"""The focal and smooth-L1 loss kernels (csrc/kernels/losses.hip, focal_common.h) in every dispatch form of
``mxr_focal_fwd_bwd`` / ``mxr_smooth_l1_fwd_bwd`` against a plain float64 restatement of SURVEY §2.8.6, per
element, on the values the kernel receives (inputs rounded to the kernel's input type first).

Not covered here: the 64-bit-index kernel ``focal_kernel<bf16_t, 8>``.  ``mxr_focal_fwd_bwd`` takes it only from
2^31 logits on -- 4.3 GB in, 4.3 GB out and a chunked float64 reference -- which is far beyond the few seconds
a test of this suite may take.
"""
import math

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops.losses import LOGIT_HI, LOGIT_LO

pytestmark = pytest.mark.gpu

ALPHA = 0.25
# the clip bounds as the kernel receives them (ctypes passes them as fp32)
LO = float(np.float32(LOGIT_LO))
HI = float(np.float32(LOGIT_HI))

# |got - ref| <= rtol |ref| + ATOL / max(1, npos), every element
ATOL = 1e-13
# bf16: one rounding to bf16 (2^-9) plus the kernel's fp32 log(1 + e) and softplus(x) - x, which lose relative
# accuracy as |x| grows: an fp32 emulation of focal_elem over every bf16 value in [-40, 40] and both classes
# stays within 2^-7 |ref| + 1e-15, and leaves 2^-7 |ref| alone only where |grad| < 1e-13
RTOL_BF16 = 2.0 ** -7
# fp32: PyTorch's own fp32 autograd (on the CPU) of the formula below (_focal_formula, on the fp32 logits of the
# two fp32 cases of this file) measured against the float64 reference with the same metric needs, with
# ATOL as above, rtol = 5.83e-7 / 7.52e-7 (C = 20, gamma 2 / 1.5) and 5.34e-7 / 7.02e-7 (C = 3): 7.52e-7 at
# worst.  The kernel gets 8x that, 6.0e-6: its exp / log1p / pow are good to an ulp or two, not correctly rounded.
RTOL_F32_TORCH = 7.52e-7
RTOL_F32 = 8 * RTOL_F32_TORCH
LOSS_RTOL = 1e-5

SL1_RTOL_BF16 = 2.0 ** -8     # 9 d / npos or +-1 / npos rounded once to bf16, plus fp32 roundings
SL1_RTOL_F32 = 2.0 ** -21     # three fp32 roundings


# ------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------
def _softplus(x):
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def _focal_formula(x, y, keep, gamma):
    """sum over kept rows of  alpha_t (1 - p | p)^gamma BCE(y, clamp(x))  in the dtype of x (unnormalised), for
    autograd: the fp32 yardstick of RTOL_F32.  p^gamma is written exp(-gamma softplus(-x)): the backward of
    torch.sigmoid is p (1 - p), which is 0 in fp32 from x = 17 on (a 100 % error in d(weight)/dx there)."""
    xc = x.clamp(LO, HI)
    w = torch.where(y, ALPHA * torch.exp(-gamma * _softplus(x)), (1 - ALPHA) * torch.exp(-gamma * _softplus(-x)))
    bce = torch.where(y, _softplus(-xc), _softplus(xc))
    return (w * bce * keep[:, None].to(x.dtype)).sum()


def focal_ref(x, state, label, npos, gamma):
    """float64 loss (python float) and per-element gradient of logits x [R, C] (any float dtype, exact in f64)."""
    x = x.double()
    R, C = x.shape
    y = (state == 1)[:, None] & (torch.arange(C, device=x.device)[None, :] == label.long()[:, None])
    keep = (state != -1)[:, None].double()
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    xc = x.clamp(LO, HI)
    inr = ((x > LO) & (x < HI)).double()
    pg, qg = p ** gamma, q ** gamma
    w = torch.where(y, ALPHA * qg, (1 - ALPHA) * pg)
    dw = torch.where(y, -ALPHA * gamma * qg * p, (1 - ALPHA) * gamma * pg * q)
    bce = torch.where(y, _softplus(-xc), _softplus(xc))
    dbce = torch.where(y, -q, p) * inr
    div = max(1, int(npos))
    loss = (w * bce * keep).sum().item() / div
    grad = (dw * bce + w * dbce) * keep / div
    return loss, grad


def smooth_l1_ref(pred, target, state, npos):
    """float64 loss and gradient [R, 4], and the gradient each element would have in the other branch."""
    d = pred.double() - target.double()
    pos = (state == 1)[:, None].double()
    ad = d.abs()
    quad = ad < 1.0 / 9.0
    div = max(1, int(npos))
    loss = (torch.where(quad, 0.5 * 9.0 * d * d, ad - 0.5 / 9.0) * pos).sum().item() / div
    g_quad, g_lin = 9.0 * d * pos / div, torch.sign(d) * pos / div
    return loss, torch.where(quad, g_quad, g_lin), torch.where(quad, g_lin, g_quad), d


# ------------------------------------------------------------------------------------------------
# assertions
# ------------------------------------------------------------------------------------------------
def _check_grad(got, ref, rtol, npos, what, alt=None, alt_mask=None):
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    atol = ATOL / max(1, int(npos))
    err = (got - ref).abs()
    ok = err <= rtol * ref.abs() + atol
    if alt is not None:
        ok |= alt_mask & ((got - alt).abs() <= rtol * alt.abs() + atol)
    need = torch.where(ref != 0, (err - atol).clamp_min(0) / ref.abs(), torch.zeros_like(err))
    print("{}: worst rtol needed {:.3e} (allowed {:.3e})".format(what, need.max().item(), rtol))
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("{}: {} of {} gradient elements off, in rows {}; first at {}: got {!r} ref {!r}".format(
            what, bad.shape[0], ok.numel(), sorted(set(bad[:, 0].tolist()))[:12], i, got[i].item(), ref[i].item()))


def _check_loss(got, ref, what):
    got = float(got)
    print("{}: loss {!r} ref {!r} rel {:.3e}".format(what, got, ref, abs(got - ref) / abs(ref) if ref else 0.0))
    assert math.isfinite(got), what
    assert abs(got - ref) <= LOSS_RTOL * abs(ref), (what, got, ref)


# ------------------------------------------------------------------------------------------------
# inputs (generated on the host: the same bits whatever the device)
# ------------------------------------------------------------------------------------------------
def _mixture(gen, shape):
    """~70 % randn * 3, 15 % uniform in (HI, 40), 15 % uniform in (-40, LO)."""
    u = torch.rand(shape, generator=gen)
    t = torch.rand(shape, generator=gen)
    x = torch.randn(shape, generator=gen) * 3
    x = torch.where(u < 0.15, HI + 0.05 + t * (40 - HI - 0.05), x)
    return torch.where(u > 0.85, LO - 0.05 - t * (40 + LO - 0.05), x)


def _planted_labels(C):
    """column 0 and C - 1, and the first / last lane of the first, an inner and the last 8- and 4-vector."""
    return sorted({c for c in (0, 3, 4, 7, 8, C - 8, C - 4, C - 1) if 0 <= c < C})


def focal_inputs(R, C, dtype, seed, states="mixed"):
    gen = torch.Generator().manual_seed(seed)
    x = _mixture(gen, (R, C))
    label = torch.randint(0, C, (R,), generator=gen).to(torch.int32)
    if states == "mixed":
        state = torch.randint(-1, 2, (R,), generator=gen).to(torch.int8)
        plant = _planted_labels(C)
        for i, c in enumerate(plant):        # at the head and at the tail of the tensor
            for r in (i, R - 1 - i):
                state[r], label[r] = 1, c
    elif states == "negative":
        state = torch.zeros(R, dtype=torch.int8)
    elif states == "ignored":
        state = torch.full((R,), -1, dtype=torch.int8)
    else:
        assert states == "one"
        state = torch.randint(-1, 1, (R,), generator=gen).to(torch.int8)
        state[R // 2] = 1
    pos = (state == 1).nonzero().flatten()
    x[pos, label[pos].long()] = _mixture(gen, (pos.numel(),))
    x = x.to(dtype)
    if states == "mixed":
        # every branch has many members, whatever a later change of the seed does
        xf, n = x.float(), x.numel()
        assert 0.12 * n < (xf > HI).sum() < 0.18 * n and 0.12 * n < (xf < LO).sum() < 0.18 * n
        xp = xf[pos, label[pos].long()]
        assert (xp < LO).sum() >= 10 and (xp > HI).sum() >= 10 and ((xp > LO) & (xp < HI)).sum() >= 50
        for s in (-1, 0, 1):
            assert 0.25 * R < (state == s).sum() < 0.42 * R
        for c in _planted_labels(C):
            assert ((state == 1) & (label == c)).sum() >= 2
    return x, state, label


def _run_focal(cuda, dtype, C, A, P, gamma, ld, seed, states="mixed", npos=None, same_body=True):
    """The plain-layout call against float64 and, with ld > 0, the padded call against float64, against the
    plain call's bits (same_body) and for untouched padding columns.  Rows = 2 x A x P."""
    R = 2 * A * P
    x, state, label = (t.to(cuda) for t in focal_inputs(R, C, dtype, seed, states))
    n = int((state == 1).sum().item()) if npos is None else npos
    npos_t = None if npos is None else torch.tensor([npos], dtype=torch.int32, device=cuda)
    ref_loss, ref_grad = focal_ref(x, state, label, n, gamma)
    rtol = RTOL_BF16 if dtype == torch.bfloat16 else RTOL_F32
    what = "focal {} C={} gamma={} {}".format(str(dtype)[6:], C, gamma, states)
    loss, grad = N.focal_fwd_bwd(x, state, label, npos=npos_t, gamma=gamma)
    assert grad.dtype == dtype and grad.shape == x.shape
    _check_grad(grad, ref_grad, rtol, n, what)
    _check_loss(loss, ref_loss, what)
    if ld:
        buf = torch.zeros(2 * P, ld, dtype=dtype, device=cuda)
        loss2, g2 = N.focal_fwd_bwd(x, state, label, npos=npos_t, gamma=gamma, grad_out=buf, group=A)
        assert g2 is buf
        sliced = buf[:, :A * C].reshape(R, C)
        _check_grad(sliced, ref_grad, rtol, n, what + " padded")
        _check_loss(loss2, ref_loss, what + " padded")
        assert not buf[:, A * C:].any(), "padding columns written"
        if same_body:
            assert torch.equal(loss2, loss)
            assert torch.equal(sliced, grad)
    return loss, grad


# ------------------------------------------------------------------------------------------------
# focal: every launch form but the 64-bit-index one
# ------------------------------------------------------------------------------------------------
FOCAL_CASES = [
    # id, dtype, C, anchors per pixel, pixels per image, ld (0: plain only), padded call runs the plain call's body
    ("bf16_c80", torch.bfloat16, 80, 9, 37, 768, True),          # focal_bf16_kernel<4,80,9,true> / <4,80,9>
    # 2,106,000 vectors > 4 x 2048 x 256: all four u lanes, the st == -2 tail guard, a second loop trip
    ("bf16_c80_big", torch.bfloat16, 80, 9, 11700, 768, True),
    ("bf16_c8", torch.bfloat16, 8, 9, 37, 128, True),            # generic focal_bf16_kernel<4> (kitti)
    ("bf16_c16", torch.bfloat16, 16, 9, 37, 192, True),
    ("bf16_c80_g15", torch.bfloat16, 80, 15, 23, 1216, False),   # generic via group != 9
    ("bf16_c20", torch.bfloat16, 20, 9, 37, 0, True),            # focal_kernel_scalar<bf16_t> (pascal)
    ("f32_c20", torch.float32, 20, 9, 37, 0, True),              # focal_kernel<float, 4>
    ("f32_c3", torch.float32, 3, 9, 37, 0, True),                # focal_kernel_scalar<float>
]


@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("case", FOCAL_CASES, ids=[c[0] for c in FOCAL_CASES])
def test_focal_forms(cuda, case, gamma):
    _, dtype, C, A, P, ld, same_body = case
    _run_focal(cuda, dtype, C, A, P, gamma, ld, seed=11 + C, same_body=same_body)


@pytest.mark.parametrize("C", [80, 20])
def test_focal_no_positives(cuda, C):
    """npos = 0: the divisor is 1, not 0."""
    loss, grad = _run_focal(cuda, torch.bfloat16, C, 9, 37, 2.0, 768 if C == 80 else 0, seed=21, states="negative")
    assert math.isfinite(loss.item()) and loss.item() > 0 and bool(torch.isfinite(grad.float()).all())


@pytest.mark.parametrize("C", [80, 20])
def test_focal_all_ignored(cuda, C):
    loss, grad = _run_focal(cuda, torch.bfloat16, C, 9, 37, 2.0, 768 if C == 80 else 0, seed=22, states="ignored")
    assert loss.item() == 0.0
    assert not grad.any()


@pytest.mark.parametrize("C", [80, 20])
def test_focal_one_positive(cuda, C):
    _run_focal(cuda, torch.bfloat16, C, 9, 37, 2.0, 768 if C == 80 else 0, seed=23, states="one")


@pytest.mark.parametrize("C", [80, 20])
def test_focal_explicit_npos(cuda, C):
    """The kernel divides by the npos it is handed (the target kernel's count over the whole local batch), not
    by the number of state-1 rows it sees."""
    _run_focal(cuda, torch.bfloat16, C, 9, 37, 2.0, 768 if C == 80 else 0, seed=24, npos=57)


def test_focal_padded_argument_checks(cuda):
    """mxr_focal_fwd_bwd refuses a padded layout it has no kernel for, before any launch."""
    R = 2 * 9 * 4
    state = torch.zeros(R, dtype=torch.int8, device=cuda)
    label = torch.zeros(R, dtype=torch.int32, device=cuda)

    def call(C, dtype, ld, group=9):
        x = torch.zeros(R, C, dtype=dtype, device=cuda)
        buf = torch.zeros(R // group, ld, dtype=dtype, device=cuda)
        N.focal_fwd_bwd(x, state, label, grad_out=buf, group=group)
        return buf

    with pytest.raises((RuntimeError, ValueError)):
        call(20, torch.bfloat16, 192)             # C % 8 != 0
    with pytest.raises((RuntimeError, ValueError)):
        call(80, torch.bfloat16, 712)             # group * C > ld
    with pytest.raises((RuntimeError, ValueError)):
        call(80, torch.float32, 768)              # fp32 grad_out
    with pytest.raises((RuntimeError, ValueError)):  # fp32 grad_out for bf16 logits
        N.focal_fwd_bwd(torch.zeros(R, 80, dtype=torch.bfloat16, device=cuda), state, label,
                        grad_out=torch.zeros(R // 9, 768, device=cuda), group=9)
    torch.cuda.synchronize()
    assert not call(80, torch.bfloat16, 768)[:, 720:].any()   # the accepted form of the same call


# ------------------------------------------------------------------------------------------------
# smooth-L1
# ------------------------------------------------------------------------------------------------
def _neighbours(v, dtype, k):
    """v moved by k representable steps of dtype (v > 0)."""
    if dtype == torch.bfloat16:
        return (torch.tensor([v], dtype=dtype).view(torch.int16) + k).view(dtype).item()
    return float((np.array([v], dtype=np.float32).view(np.int32) + k).view(np.float32)[0])


def sl1_inputs(R, dtype, seed, states="mixed"):
    gen = torch.Generator().manual_seed(seed)
    pred = (torch.randn(R, 4, generator=gen) * 0.3)
    target = torch.randn(R, 4, generator=gen) * 0.3
    if states == "mixed":
        state = torch.randint(-1, 2, (R,), generator=gen).to(torch.int8)
    elif states == "negative":
        state = torch.randint(-1, 1, (R,), generator=gen).to(torch.int8)
    else:
        state = torch.full((R,), -1, dtype=torch.int8)
    planted = torch.zeros(R, dtype=torch.bool)
    if states == "mixed":
        thr = torch.tensor([1.0 / 9.0]).to(dtype).item()          # 1/9 rounded to the input type
        vals = [0.0, 50.0] + [_neighbours(thr, dtype, k) for k in (-2, -1, 0, 1, 2)]
        vals = [s * v for v in vals for s in (1.0, -1.0)]
        rows = (len(vals) + 3) // 4
        v = torch.tensor(vals + [0.0] * (rows * 4 - len(vals)), dtype=torch.float64).reshape(rows, 4)
        for r0 in (0, R - rows):                                   # difference = prediction: target 0
            pred[r0:r0 + rows] = v.float()
            target[r0:r0 + rows] = 0
            state[r0:r0 + rows] = 1
            planted[r0:r0 + rows] = True
    pred = pred.to(dtype)
    if states == "mixed":
        d = (pred.double() - target.double()).abs()[state == 1]
        assert (d < 1 / 9).sum() > 0.1 * d.numel() and (d >= 1 / 9).sum() > 0.3 * d.numel()
        assert (d == 0).sum() >= 4 and (d == 50).sum() >= 4
    return pred, target, state, planted


def _run_sl1(cuda, dtype, P, seed, states="mixed", npos=None):
    A, ld = 9, 64
    R = 2 * A * P
    pred, target, state, planted = (t.to(cuda) for t in sl1_inputs(R, dtype, seed, states))
    n = int((state == 1).sum().item()) if npos is None else npos
    npos_t = None if npos is None else torch.tensor([npos], dtype=torch.int32, device=cuda)
    ref_loss, ref_grad, other, d = smooth_l1_ref(pred, target, state, n)
    # a planted row within one input ulp of the threshold may take either branch
    ulp = 2.0 ** -11 if dtype == torch.bfloat16 else 2.0 ** -27      # ulp of the input type at 1/9
    near = planted[:, None] & ((d.abs() - 1.0 / 9.0).abs() <= ulp)
    if states == "mixed":
        assert 4 <= int(near.sum().item()) <= 2 * 6
    rtol = SL1_RTOL_BF16 if dtype == torch.bfloat16 else SL1_RTOL_F32
    what = "smooth_l1 {} rows={} {}".format(str(dtype)[6:], R, states)
    loss, grad = N.smooth_l1_fwd_bwd(pred, target, state, npos=npos_t)
    assert grad.dtype == dtype and grad.shape == pred.shape
    _check_grad(grad, ref_grad, rtol, n, what, alt=other, alt_mask=near)
    _check_loss(loss, ref_loss, what)
    buf = torch.zeros(2 * P, ld, dtype=dtype, device=cuda)
    loss2, g2 = N.smooth_l1_fwd_bwd(pred, target, state, npos=npos_t, grad_out=buf, group=A)
    assert g2 is buf
    sliced = buf[:, :A * 4].reshape(R, 4)
    _check_grad(sliced, ref_grad, rtol, n, what + " padded", alt=other, alt_mask=near)
    _check_loss(loss2, ref_loss, what + " padded")
    assert not buf[:, A * 4:].any(), "padding columns written"
    assert torch.equal(loss2, loss) and torch.equal(sliced, grad)
    if states == "mixed":
        assert not grad[(d == 0)].any()          # a zero difference has exactly zero gradient
    return loss, grad


@pytest.mark.parametrize("dtype,P", [(torch.bfloat16, 37), (torch.float32, 37),
                                     (torch.bfloat16, 33000)],   # 594,000 rows > 2048 x 256 threads
                         ids=["bf16", "f32", "bf16_big"])
def test_smooth_l1_forms(cuda, dtype, P):
    _run_sl1(cuda, dtype, P, seed=31)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_smooth_l1_no_positives(cuda, dtype):
    loss, grad = _run_sl1(cuda, dtype, 37, seed=32, states="negative")
    assert loss.item() == 0.0 and not grad.any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_smooth_l1_all_ignored(cuda, dtype):
    loss, grad = _run_sl1(cuda, dtype, 37, seed=33, states="ignored")
    assert loss.item() == 0.0 and not grad.any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_smooth_l1_explicit_npos(cuda, dtype):
    _run_sl1(cuda, dtype, 37, seed=34, npos=57)
