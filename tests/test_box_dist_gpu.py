"""The kernels of csrc/kernels/box_dist.hip (through ``native.box_integral_fwd`` / ``native.box_dist_fwd_bwd``) per
element against float64: the float64 autograd of the formulas as restated below (independently of ops/boxes.py and
ops/losses.py), on the values the kernels receive (logits and delta gradients rounded to their input type first).

Inputs: B = 2 images of 45 locations x 9 anchors, 810 rows -- not a multiple of a tile's 63 (padded layout) or 64
(plain layout) rows, so the last tile is short.  About 10 % of the rows are positive, about 10 % have state -1.
logits = 2 randn, targets = 3 randn (a few beyond +-R), delta gradients = randn / positives.  The first positive
rows carry the special cases: targets exactly on bin values, targets far beyond both ends, one logit of +80 or -80 in
a side, all logits of a side equal.  K in {17, 8, 16, 5}: the compile-time form, the run-time form with padded rows
(9 * 4 * 8 = 288 -> 320), the form whose plain layout is the final layer's (9 * 4 * 16 = 576) and an odd small K.

Metric.  The K gradient elements of a side cancel (both terms sum to 0 over the bins), so the bound is on the side's
scale g = max_i |ref[row, side, i]|; the integral's error scale is the range R (the products p_i v_i cancel):
    fp32   |got - ref| <= RTOL32 * g                  |y - ref| <= RTOL32_FWD * R
    bf16   |got - ref| <= 2^-8 |ref| + RTOL32 * g     |y - ref| <= 2^-8 |ref| + RTOL32_FWD * R     (one rounding)
Yardstick: PyTorch's own fp32 autograd (on the CPU) of the same formulas (``_formula`` below, in fp32) on this
file's inputs against the float64 reference under this metric needs, over the four K and fp32 / bf16-rounded inputs,
    gradient  5.45e-7 .. 3.20e-6      integral  1.71e-7 .. 3.20e-7
(62 .. 88 positive rows; the loss itself is within 1.1e-7 relative).  The kernels get 8x the worst of each, 2.56e-5
and 2.56e-6, the margin test_iou_loss_gpu.py gives its kernel and for its reason: expf, logf and the reciprocal are
good to an ulp or two, not correctly rounded.  The scalar loss agrees with float64 to 1e-5 relative, as in that file.
"""
import functools
import math

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import boxes as box_ops
from batchai_retinanet_horovod_coco_amd.ops import losses
from batchai_retinanet_horovod_coco_amd.ops import native as N

pytestmark = pytest.mark.gpu

CASES = [(17, 8.0), (8, 8.0), (16, 8.0), (5, 3.0)]
DTYPES = [torch.float32, torch.bfloat16]
B, LOC, GROUP = 2, 45, 9
ROWS = B * LOC * GROUP
WEIGHT = 0.25
RTOL_BF16 = 2.0 ** -8
LOSS_RTOL = 1e-5
SENTINEL = 12288.0          # exact in bf16
GUARD = 64                  # elements in front of and behind a guarded buffer (keeps 16-byte alignment)


def _ld(K):
    return (GROUP * 4 * K + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------
def _formula(logits, dreg, target, pos, npos, K, R, weight):
    """(y [rows, 4], DFL loss, the scalar whose gradient w.r.t. the logits box_dist.hip writes) in the logits' dtype."""
    dt = logits.dtype
    l = logits.reshape(-1, 4, K)
    D = 2.0 * R / (K - 1)
    v = -R + torch.arange(K, dtype=torch.float64) * D
    v = v.to(dt)
    m = l.max(-1, keepdim=True).values
    e = torch.exp(l - m)
    S = e.sum(-1, keepdim=True)
    y = (e / S * v).sum(-1)
    logp = (l - m) - torch.log(S)
    u = ((target.to(dt) + R) / D).clamp(0, (K - 1) - 0.01)
    il = u.floor()
    wr = u - il
    il = il.long()
    per = -((1 - wr) * logp.gather(-1, il[..., None])[..., 0] + wr * logp.gather(-1, il[..., None] + 1)[..., 0])
    mask = pos[:, None].to(dt)
    dfl = weight * (per * mask).sum() / (4 * max(1, npos))
    return y, dfl, dfl + (dreg.to(dt) * y * mask).sum()


def reference(logits, dreg, target, state, npos, K, R, weight=WEIGHT, dtype=torch.float64):
    """y, DFL loss (python float), dlogits [rows, 4, K]; ``dtype=torch.float32`` is the yardstick."""
    l = logits.to(dtype).requires_grad_(True)
    y, dfl, total = _formula(l, dreg, target, state == 1, npos, K, R, weight)
    total.backward()
    return y.detach(), dfl.item(), l.grad.reshape(-1, 4, K)


def grad_need(got, ref, pos, rel=0.0):
    """The RTOL32 the positive rows need: max over their elements of (|got - ref| - rel |ref|) / g_side."""
    ref = ref[pos]
    err = (got.double().reshape(-1, *ref.shape[1:])[pos] - ref).abs() - rel * ref.abs()
    scale = ref.abs().max(-1, keepdim=True).values
    assert bool((scale > 0).all())
    return (err / scale).max().clamp_min(0).item() if ref.numel() else 0.0


def fwd_need(got, ref, R, rel=0.0):
    err = (got.double() - ref).abs() - rel * ref.abs()
    return (err / R).max().clamp_min(0).item() if ref.numel() else 0.0


# ------------------------------------------------------------------------------------------------
# inputs (generated on the host: the same bits whatever the device)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(K, R, dtype, seed=0):
    """logits [ROWS, 4K] dtype, dreg [ROWS, 4] dtype, target [ROWS, 4] f32, state [ROWS] int8 (on the host)."""
    g = torch.Generator().manual_seed(100 * K + seed)
    logits = 2 * torch.randn(ROWS, 4 * K, generator=g)
    target = 3 * torch.randn(ROWS, 4, generator=g) * (R / 8.0)
    r = torch.rand(ROWS, generator=g)
    state = torch.where(r < 0.1, 1, torch.where(r < 0.2, -1, 0)).to(torch.int8)
    state[ROWS - 1] = 1                              # the short last tile has a positive row
    pos = (state == 1).nonzero().flatten()
    assert 60 <= pos.numel() <= 110 and int((state == -1).sum()) >= 40
    D = 2 * R / (K - 1)
    p = pos.tolist()
    target[p[0]] = torch.tensor([-R, -R + D, R - D, -R + (K // 2) * D])          # on bin values
    target[p[1]] = torch.tensor([-3 * R, 5 * R, R, -R - 1e-3])                   # beyond both ends, and the last value
    logits[p[2], 1] = 80.0
    logits[p[2], K + 2] = -80.0
    logits[p[2], 2 * K:3 * K] = 0.75                                             # a side of equal logits
    logits[p[2], 3 * K:4 * K] = -80.0
    logits[p[3], K - 1] = 80.0                                                   # all the mass on the last bin ...
    target[p[3], 0] = -R                                                         # ... the target on the first
    logits[p[4], 0:K] = 80.0
    logits[p[4], 0] = -80.0
    dreg = torch.randn(ROWS, 4, generator=g) / pos.numel()
    return logits.to(dtype), dreg.to(dtype), target, state


def yardstick():
    """What fp32 CPU autograd needs under this file's metric (run on the host; the numbers are in the docstring)."""
    out = {}
    for K, R in CASES:
        for dtype in DTYPES:
            logits, dreg, target, state = inputs(K, R, dtype)
            npos = int((state == 1).sum())
            y64, l64, g64 = reference(logits, dreg, target, state, npos, K, R)
            y32, l32, g32 = reference(logits, dreg, target, state, npos, K, R, dtype=torch.float32)
            out[(K, str(dtype)[6:])] = (grad_need(g32, g64, state == 1), fwd_need(y32, y64, R),
                                        abs(l32 - l64) / abs(l64), npos)
    return out


# measured with yardstick(): see the module docstring
RTOL32_TORCH = 3.20e-6
RTOL32_FWD_TORCH = 3.20e-7
RTOL32 = 8 * RTOL32_TORCH
RTOL32_FWD = 8 * RTOL32_FWD_TORCH


def _guarded(numel, dtype, dev):
    """A 16-byte-aligned buffer of ``numel`` sentinels with guard elements in front and behind."""
    full = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    return full, full[GUARD:GUARD + numel]


def _guards_intact(full, numel):
    return bool((full[:GUARD] == SENTINEL).all()) and bool((full[GUARD + numel:] == SENTINEL).all())


def _check_loss(got, ref, what):
    got = float(got.detach())
    print("{}: loss {!r} ref {!r} rel {:.3e}".format(what, got, ref, abs(got - ref) / abs(ref) if ref else 0.0))
    assert math.isfinite(got), what
    assert abs(got - ref) <= LOSS_RTOL * abs(ref), (what, got, ref)


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("K,R", CASES)
def test_loss_and_gradient_against_float64(cuda, K, R, dtype):
    logits, dreg, target, state = inputs(K, R, dtype)
    npos = int((state == 1).sum())
    _, ref_loss, ref_grad = reference(logits, dreg, target, state, npos, K, R)
    d = [t.to(cuda) for t in (logits, dreg, target, state)]
    rel = RTOL_BF16 if dtype == torch.bfloat16 else 0.0
    what = "K={} {}".format(K, str(dtype)[6:])
    # plain layout, written into a guarded buffer
    W = 4 * K
    loss, grad = N.box_dist_fwd_bwd(*d, K=K, R=R, weight=WEIGHT)
    assert grad.dtype == dtype and grad.shape == logits.shape
    g = grad.cpu().reshape(ROWS, 4, K)
    need = grad_need(g, ref_grad, state == 1, rel)
    print("{}: worst RTOL32 needed {:.3e} (allowed {:.3e}) over {} positive rows".format(what, need, RTOL32, npos))
    assert not g[state != 1].any(), what + ": a row that is not positive has a gradient"
    assert bool(torch.isfinite(g.float()).all()), what
    assert need <= RTOL32, (what, need)
    _check_loss(loss, ref_loss, what)
    # two calls give the same bits
    loss_b, grad_b = N.box_dist_fwd_bwd(*d, K=K, R=R, weight=WEIGHT)
    assert torch.equal(loss, loss_b) and torch.equal(grad, grad_b)
    # the padded layout: the same gradient bits, padding columns and the memory around the buffer untouched
    ld = _ld(K)
    full, flat = _guarded(ROWS // GROUP * ld, dtype, cuda)
    buf = flat.view(ROWS // GROUP, ld)
    loss_p, gp = N.box_dist_fwd_bwd(*d, K=K, R=R, weight=WEIGHT, grad_out=buf, group=GROUP)
    torch.cuda.synchronize()
    assert gp is buf and _guards_intact(full, flat.numel())
    assert bool((buf[:, GROUP * W:] == SENTINEL).all()), "padding columns written"
    assert torch.equal(buf[:, :GROUP * W].reshape(ROWS, W), grad)
    # (the loss is summed per tile, 63 rows here and 64 in the plain layout: the same value, not the same bits)
    _check_loss(loss_p, ref_loss, what + " padded")
    loss_q, _ = N.box_dist_fwd_bwd(*d, K=K, R=R, weight=WEIGHT, grad_out=torch.zeros_like(buf), group=GROUP)
    assert torch.equal(loss_p, loss_q)
    if (GROUP * W) % 64 == 0:
        # K = 16: the plain layout is the final layer's own
        assert ld == GROUP * W and torch.equal(grad.reshape(ROWS // GROUP, ld), buf)
    # a wider pitch, and the plain layout at the end of an allocation
    full2, flat2 = _guarded(ROWS // GROUP * (ld + 64), dtype, cuda)
    N.box_dist_fwd_bwd(*d, K=K, R=R, weight=WEIGHT, grad_out=flat2.view(ROWS // GROUP, ld + 64), group=GROUP)
    full3, flat3 = _guarded(ROWS * W, dtype, cuda)
    rc = N.lib().mxr_box_dist_fwd_bwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      torch.tensor([npos], dtype=torch.int32, device=cuda).data_ptr(), flat3.data_ptr(),
                                      torch.empty(N.LOSS_GRID, device=cuda).data_ptr(), torch.empty(1, device=cuda).data_ptr(),
                                      ROWS, K, R, WEIGHT, 1 if dtype == torch.bfloat16 else 0, 0, 0,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and _guards_intact(full2, flat2.numel()) and _guards_intact(full3, flat3.numel())
    assert torch.equal(flat2.view(ROWS // GROUP, ld + 64)[:, :GROUP * W].reshape(ROWS, W), grad)
    assert bool((flat2.view(ROWS // GROUP, ld + 64)[:, GROUP * W:] == SENTINEL).all())
    assert torch.equal(flat3.view(ROWS, W), grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("K,R", CASES)
def test_integral_against_float64(cuda, K, R, dtype):
    logits, dreg, target, state = inputs(K, R, dtype)
    ref_y, _, _ = reference(logits, dreg, target, state, 1, K, R)
    rel = RTOL_BF16 if dtype == torch.bfloat16 else 0.0
    what = "K={} {}".format(K, str(dtype)[6:])
    dl, ds = logits.to(cuda), state.to(cuda)
    # every row (the prediction model's form)
    y = N.box_integral_fwd(dl, K, R)
    assert y.dtype == dtype and y.shape == (ROWS, 4)
    need = fwd_need(y.cpu(), ref_y, R, rel)
    print("{}: integral, worst RTOL32_FWD needed {:.3e} (allowed {:.3e})".format(what, need, RTOL32_FWD))
    assert bool(torch.isfinite(y.float()).all()) and need <= RTOL32_FWD, (what, need)
    assert torch.equal(y, N.box_integral_fwd(dl, K, R))
    # logits that are not 16-byte aligned take the per-lane loads: the same bits
    off = torch.empty(dl.numel() + 1, dtype=dtype, device=cuda)
    off[1:] = dl.reshape(-1)
    assert off[1:].data_ptr() % 16 != 0
    assert torch.equal(y, N.box_integral_fwd(off[1:].view(ROWS, 4 * K), K, R))
    # positive rows only (the training form): their values are the all-rows values, every other row is exactly 0
    yt = N.box_integral_fwd(dl, K, R, state=ds)
    pos = ds == 1
    assert torch.equal(yt[pos], y[pos]) and not yt[~pos].any()
    assert torch.equal(yt, N.box_integral_fwd(dl, K, R, state=ds))
    # the output's surroundings
    for st in (None, ds):
        full = torch.full((ROWS * 4 + 2 * GUARD,), SENTINEL, dtype=dtype, device=cuda)
        rc = N.lib().mxr_box_integral_fwd(dl.data_ptr(), None if st is None else st.data_ptr(),
                                          full[GUARD:].data_ptr(), ROWS, K, R, 1 if dtype == torch.bfloat16 else 0,
                                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and _guards_intact(full, ROWS * 4)
        assert torch.equal(full[GUARD:GUARD + ROWS * 4].view(ROWS, 4), y if st is None else yt)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_no_positives(cuda, dtype):
    K, R = 17, 8.0
    logits, dreg, target, state = inputs(K, R, dtype)
    state = torch.where(state == 1, torch.zeros_like(state), state)
    d = [t.to(cuda) for t in (logits, dreg, target, state)]
    loss, grad = N.box_dist_fwd_bwd(*d, K=K, R=R, weight=WEIGHT)
    buf = torch.full((ROWS // GROUP, _ld(K)), SENTINEL, dtype=dtype, device=cuda)
    loss_p, _ = N.box_dist_fwd_bwd(*d, K=K, R=R, weight=WEIGHT, grad_out=buf, group=GROUP)
    assert float(loss) == 0.0 and float(loss_p) == 0.0 and not grad.any()
    assert not buf[:, :GROUP * 4 * K].any() and bool((buf[:, GROUP * 4 * K:] == SENTINEL).all())
    assert not N.box_integral_fwd(d[0], K, R, state=d[3]).any()
    # npos read from device memory: a count of 0 next to positive rows divides by max(1, .)
    logits, dreg, target, state = (t.to(cuda) for t in inputs(K, R, dtype))
    zero = torch.zeros(1, dtype=torch.int32, device=cuda)
    n = int((state == 1).sum())
    l0, _ = N.box_dist_fwd_bwd(logits, dreg, target, state, npos=zero, K=K, R=R, weight=WEIGHT)
    l1, _ = N.box_dist_fwd_bwd(logits, dreg, target, state, K=K, R=R, weight=WEIGHT)
    assert abs(float(l0) - n * float(l1)) <= 1e-5 * float(l0)


def test_wrappers_and_autograd(cuda):
    """``box_integral`` and ``distribution_focal_loss`` on the GPU run the kernels and backpropagate."""
    K, R = 17, 8.0
    logits, dreg, target, state = (t.to(cuda) for t in inputs(K, R, torch.float32))
    npos = int((state == 1).sum())
    ref_y, ref_loss, _ = reference(logits.cpu(), torch.zeros_like(dreg).cpu(), target.cpu(), state.cpu(), npos, K, R)
    l = logits.reshape(B, -1, 4 * K).clone().requires_grad_(True)
    y = box_ops.box_integral(l, K, R)
    assert isinstance(y.grad_fn, N.BoxIntegralFn._backward_cls) and y.shape == (B, ROWS // B, 4)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(cuda)
    y.backward(gy)
    l64 = logits.cpu().double().reshape(B, -1, 4 * K).requires_grad_(True)
    y64, _, _ = _formula(l64, torch.zeros(ROWS, 4), target.cpu(), torch.zeros(ROWS, dtype=torch.bool), 1, K, R, 0.0)
    y64.backward(gy.cpu().double().reshape(-1, 4))
    assert fwd_need(y.detach().cpu().reshape(-1, 4), ref_y, R) <= RTOL32_FWD
    assert torch.allclose(l.grad.cpu().double(), l64.grad, rtol=1e-4, atol=1e-6)
    l2 = logits.reshape(B, -1, 4 * K).clone().requires_grad_(True)
    loss = losses.distribution_focal_loss(l2, target.reshape(B, -1, 4), state.reshape(B, -1), K, R, WEIGHT)
    assert isinstance(loss.grad_fn, N.DistributionFocalLossFn._backward_cls)
    _check_loss(loss, ref_loss, "distribution_focal_loss")
    loss.backward()
    want = torch.autograd.grad(losses.distribution_focal_loss(l64, target.cpu().reshape(B, -1, 4),
                                                              state.cpu().reshape(B, -1), K, R, WEIGHT), l64)[0]
    assert torch.allclose(l2.grad.cpu().double(), want, rtol=1e-4, atol=1e-7)


def test_refusals_fall_back_to_the_torch_expression(cuda):
    stream = torch.cuda.current_stream().cuda_stream

    def entry(K, dtype=1, grp=0, ld=0, R=8.0, rows=18):
        Kb = max(K, 1)
        x = torch.zeros(rows * 4 * Kb + 64, dtype=torch.bfloat16, device=cuda)
        y = torch.full((rows * max(ld, 4 * Kb) + 64,), SENTINEL, dtype=torch.float32, device=cuda)
        f = torch.full((4096,), SENTINEL, dtype=torch.float32, device=cuda)
        st = torch.ones(rows, dtype=torch.int8, device=cuda)
        n = torch.ones(1, dtype=torch.int32, device=cuda)
        rc = N.lib().mxr_box_integral_fwd(x.data_ptr(), st.data_ptr(), y.data_ptr(), rows, K, R, dtype, stream)
        rb = N.lib().mxr_box_dist_fwd_bwd(x.data_ptr(), x.data_ptr(), f[3000:].data_ptr(), st.data_ptr(), n.data_ptr(),
                                          y.data_ptr(), f.data_ptr(), f[2048:].data_ptr(), rows, K, R, 0.25, dtype, grp,
                                          ld, stream)
        torch.cuda.synchronize()
        untouched = bool((y == SENTINEL).all()) and bool((f == SENTINEL).all())
        return rc, rb, untouched

    assert entry(1) == (-1, -1, True)
    assert entry(33) == (-1, -1, True)
    assert entry(17, dtype=2) == (-1, -1, True)
    assert entry(17, R=0.0) == (-1, -1, True)
    assert entry(17, grp=9, ld=608)[1:] == (-1, False)      # a pitch below the group's 612 values (the integral ran)
    assert entry(5, grp=9, ld=188)[1] == -1                 # bf16 rows of 376 bytes do not start on 16 bytes
    assert entry(17, grp=7, ld=640)[1] == -1                # rows not a multiple of the group
    rc, rb, untouched = entry(17, grp=9, ld=640)
    assert rc == 0 and rb == 0 and not untouched            # the served form runs

    g = torch.Generator().manual_seed(5)
    state = torch.tensor([[1, 0, -1, 1]], dtype=torch.int8, device=cuda)
    target = torch.randn(1, 4, 4, generator=g).to(cuda)
    for K, dt in ((17, torch.float16), (17, torch.float64)):
        x = torch.randn(1, 4, 4 * K, generator=g).to(cuda, dt).requires_grad_(True)
        box_ops._FALLBACK_WARNED.discard(("integral", K, dt))
        losses._FALLBACK_WARNED.discard(("dfl", K, dt))
        with pytest.warns(UserWarning, match="box_dist.hip does not serve"):
            y = box_ops.box_integral(x, K, 8.0)
        with pytest.warns(UserWarning, match="box_dist.hip does not serve"):
            loss = losses.distribution_focal_loss(x, target, state, K, 8.0)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")              # one warning per form
            y = box_ops.box_integral(x, K, 8.0)
            loss = losses.distribution_focal_loss(x, target, state, K, 8.0)
        assert y.dtype == dt and torch.equal(y, box_ops.box_integral(x, K, 8.0, backend="torch"))
        assert torch.equal(loss, losses.distribution_focal_loss(x, target, state, K, 8.0, backend="torch"))
        (y.float().sum() + loss.float()).backward()
        assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all())


@pytest.mark.parametrize("bins", [17, 16])
def test_model_agrees_with_the_torch_backend(cuda, bins):
    """The whole model, bf16, ``regression_bins=17`` with GIoU and QFL: one training step on the fused path (packed
    HIP heads, positive-rows integral, box_dist.hip into the final's padded rows; with 16 bins the final's 576 outputs
    need no padding and the plain layout goes through autograd) against the torch backend on the same weights and
    batch, with test_group_norm_gpu.py's bars; and the prediction model on the all-rows integral."""
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    from batchai_retinanet_horovod_coco_amd.ops import conv as conv_ops
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer

    torch.manual_seed(0)
    ref_model = models.backbone("resnet18").retinanet(8, regression_bins=bins)
    with torch.no_grad():
        # a head that says something: distributions away from uniform
        ref_model.regression_submodel.final.weight.mul_(20.0)
        ref_model.regression_submodel.final.bias.add_(torch.randn_like(ref_model.regression_submodel.final.bias))
    state = {k: v.clone() for k, v in ref_model.state_dict().items()}
    batch = make_batch(1, 128, 192, num_classes=8, generator=torch.Generator().manual_seed(7))

    def run(hip):
        if hip:
            N.enable()
            conv_ops.set_conv_backend("auto")
        else:
            N.disable()
            conv_ops.set_conv_backend("torch")
        try:
            model = models.backbone("resnet18").retinanet(8, regression_bins=bins)
            model.load_state_dict(state)
            tr = Trainer(model, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda, regression_loss="giou",
                         classification_loss="qfl")
            tr.optimizer.zero_grad()
            b = {k: v.to(cuda) for k, v in batch.items()}
            reg, cls = tr.forward_backward(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            torch.cuda.synchronize()
            grads = {s.name: tr.flat.grad[s.offset:s.offset + s.numel].double().clone() for s in tr.flat.segments}
            tr.optimizer.remove_hooks()
            extra = None
            if hip:
                assert model.reg_pad_sink is not None               # the packed heads ran
                model.eval()
                x = b["images"].to(torch.bfloat16)
                with torch.no_grad():
                    out = model(x)
                    det = models.retinanet_bbox(model)(x)
                extra = (out, det, tr.anchors.get((128, 192), cuda, None))
            return float(reg), float(cls), grads, extra
        finally:
            N.set_grad_sinks(None)
            N.set_compute_weights(None)
            N.enable()
            conv_ops.set_conv_backend("auto")

    r_t, c_t, g_t, _ = run(False)
    r_h, c_h, g_h, (out, det, anchors) = run(True)
    print("\nlosses torch bf16: reg {:.5f} cls {:.5f} | HIP bf16: reg {:.5f} cls {:.5f}".format(r_t, c_t, r_h, c_h))
    assert abs(r_h - r_t) <= 0.02 * abs(r_t) and abs(c_h - c_t) <= 0.02 * abs(c_t)
    names = [n for n in g_t if n.startswith("regression_submodel.") and (".final." in n or ".tower.0." in n or
                                                                         ".tower.3." in n)]
    assert len(names) == 6
    for name in names:
        a, b = g_t[name], g_h[name]
        assert bool(b.any()), name
        c = float(torch.dot(a, b) / (a.norm() * b.norm()))
        print("{:45s} cosine {:.5f}".format(name, c))
        assert c >= 0.95, name
    # prediction: the deltas are the all-rows kernel's integral of the logits, and the detections are those of the
    # unchanged filter on them
    logits, reg = out["regression_logits"], out["regression"]
    assert reg.dtype == torch.bfloat16 and reg.shape == logits.shape[:2] + (4,)
    want = box_ops.box_integral(logits.float(), bins, 8.0, backend="torch")
    assert float(want.abs().max()) > 1.0                            # not the uniform head's zeros
    assert bool(((reg.float() - want).abs() <= RTOL_BF16 * want.abs() + RTOL32_FWD * 8.0).all())
    boxes, scores, labels = det
    rb, rs, rl = N.filter_detections_batched(anchors, reg, out["classification"], 128, 192, 0.05, 0.5, 300)
    assert torch.equal(boxes, rb) and torch.equal(scores, rs) and torch.equal(labels, rl)
