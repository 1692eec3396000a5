"""The sparse regression-tower backward (csrc/kernels/row_activity.hip, conv_hx32.hip ACT, conv_wgrad_p8.hip SP):

* the bit kernels against ``(dy != 0).any(-1)``, ``max_pool2d`` and the numpy tile-activity rule (ops/halo.py);
* every hx32 variant's data gradient walking the active-tile list against its own dense launch, ``torch.equal``, in
  the plain, bitmask-masked, bf16-masked and accumulate forms;
* the phase-pipelined weight gradient (+ fused bias) with the row mask against its dense launch, ``torch.equal``;
* the dense results against an fp32 PyTorch reference (tests/test_proj_fused_gpu.py's tolerance);
* one small training step with the switch on and off: the same losses and ``torch.equal`` flat gradients."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GEOMS = {
    # width 100: column-split boxes (COLMAX 84)
    "wide": (2, ((20, 100), (10, 50), (5, 25), (3, 13), (2, 7))),
    # 382 rows per image, no multiple of 64: K-tiles straddle levels and images
    "ragged": (3, ((13, 21), (7, 11), (4, 6), (2, 3), (1, 2))),
}
PATTERNS = ("zero", "first", "last", "edge_out", "edge_in", "random", "all")
CIN = 256
COUTS = (256, 36)      # a tower layer; the regression final, its gradient rows padded to 64


def _rows(N, shapes):
    return N * sum(h * w for h, w in shapes)


def _support(name, N, shapes, tab):
    """bool [M]: the rows of the gradient that are non-zero."""
    M = _rows(N, shapes)
    s = np.zeros(M, dtype=bool)
    if name == "first":
        s[0] = True                      # pixel (0, 0) of image 0, level 0
    elif name == "last":
        s[M - 1] = True                  # the last pixel of the last level of the last image
    elif name in ("edge_out", "edge_in"):
        # one row on either side of a box boundary (a column boundary where the level is split by columns, else a row
        # boundary): from outside, only the neighbour's halo sees it
        from batchai_retinanet_horovod_coco_amd.ops import halo
        boxes = [b for row in tab for b in halo._boxes(row)]
        cand = [b for b in boxes if b[7] > 0] or [b for b in boxes if b[6] > 0]
        sbeg, hoff, ib, ob, H, W, y0, x0, R, C = cand[len(cand) // 2]
        if x0 > 0:
            y, x = y0, (x0 - 1 if name == "edge_out" else x0)
        else:
            y, x = (y0 - 1 if name == "edge_out" else y0), x0
        s[ob + y * W + x] = True
    elif name == "random":
        s = np.random.default_rng(3).random(M) < 0.01
        s[M // 2] = True
    elif name == "all":
        s[:] = True
    return s


def _grad(support, ld, cout, cuda, seed=0):
    """bf16 [M, ld]: random rows on the support (columns past cout zero), exact zeros elsewhere."""
    g = torch.Generator(device=cuda).manual_seed(seed)
    M = len(support)
    dy = torch.randn(M, ld, device=cuda, generator=g)
    dy[:, cout:] = 0
    dy = (dy * torch.from_numpy(support).to(cuda)[:, None]).bfloat16()
    if support.any():
        dy[np.nonzero(support)[0][0], 0] = 1.0      # a row of the support is never all zero after rounding
    return dy.contiguous()


def _levels(t, N, shapes):
    """packed [M, C] -> per level [N, C, h, w] (fp32)."""
    img = sum(h * w for h, w in shapes)
    v = t.float().reshape(N, img, -1)
    out, off = [], 0
    for h, w in shapes:
        out.append(v[:, off:off + h * w].reshape(N, h, w, -1).permute(0, 3, 1, 2))
        off += h * w
    return out


def _pack(levels):
    return torch.cat([l.permute(0, 2, 3, 1).reshape(l.shape[0], -1, l.shape[1]) for l in levels], dim=1).reshape(
        -1, levels[0].shape[1])


def _activity(dy, N, shapes, depth=0):
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    ch = RA.GradChain(depth)
    ch.start(dy, N, shapes)
    assert ch.acts is not None
    return ch


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_bit_kernels(cuda, geom):
    from batchai_retinanet_horovod_coco_amd.ops import halo
    N, shapes = GEOMS[geom]
    M = _rows(N, shapes)
    tab = halo.build_tiles(N, shapes)
    for name in PATTERNS:
        sup = _support(name, N, shapes, tab)
        dy = _grad(sup, 64, 36, cuda)
        if name == "random":
            z = int(np.nonzero(~sup)[0][0])
            dy[z, 5] = -0.0                          # a negative zero is a zero
        depth = 4
        ch = _activity(dy, N, shapes, depth)
        torch.cuda.synchronize()
        want = (dy != 0).any(-1)
        assert torch.equal(want.cpu(), torch.from_numpy(sup))
        cur = want
        for k in range(depth + 1):
            act = ch.level(k)
            got = halo.unpack_row_bits(act.words.cpu().numpy(), M)
            assert np.array_equal(got, cur.cpu().numpy()), (name, k)
            assert np.array_equal(act.words.cpu().numpy().view(np.uint64), halo.pack_row_bits(got)), (name, k)
            ref = halo.active_tiles(tab, got)
            order = act.order.cpu().numpy()
            cnt = int(act.count.item())
            assert cnt == int(ref.sum()), (name, k)
            assert np.array_equal(np.sort(order[:cnt]), np.nonzero(ref)[0]), (name, k)
            assert np.array_equal(np.sort(order), np.arange(len(tab))), (name, k)
            # the next layer's support: max_pool2d per image and level
            cur = _pack([F.max_pool2d(l, 3, 1, 1) for l in _levels(cur[:, None], N, shapes)])[:, 0] > 0


def _conv_ref(x, w, N, shapes):
    """fp32 3x3 / 'same' conv of the packed bf16 x [M, cin] with w [cout, 3, 3, cin] per level -> [M, cout]."""
    wt = w.float().permute(0, 3, 1, 2)
    return _pack([F.conv2d(l, wt, padding=1) for l in _levels(x, N, shapes)])


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_dgrad_active_list_equals_dense(cuda, geom, cout):
    """dX = conv(dY, flipped W) over cin_d = the (padded) gradient channels, cout_d = 256."""
    from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL
    from batchai_retinanet_horovod_coco_amd.ops import halo
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    N, shapes = GEOMS[geom]
    M = _rows(N, shapes)
    tab = halo.build_tiles(N, shapes)
    ld = (cout + 63) // 64 * 64
    g = CL.geom_pyramid(N, shapes, ld, CIN)
    gen = torch.Generator(device=cuda).manual_seed(11)
    w = (torch.randn(CIN, 3, 3, ld, device=cuda, generator=gen) / (9 * cout) ** 0.5).bfloat16().contiguous()
    relu_out = torch.randn(M, CIN, device=cuda, generator=gen).relu().bfloat16()
    bits = CL.BitMask.of(relu_out)
    base = torch.randn(M, CIN, device=cuda, generator=gen).bfloat16()
    variants = CL.hx32_variants(g)
    assert set(variants) >= {0, 2, 3, 4, 6, 10, 11, 13, 14}        # persistent and non-persistent, both MFMA shapes
    n0 = RA.LAUNCHES["dgrad"]
    for name in PATTERNS:
        sup = _support(name, N, shapes, tab)
        dy = _grad(sup, ld, cout, cuda)
        act = _activity(dy, N, shapes).level(0)
        ref = _conv_ref(dy, w, N, shapes) if name in ("random", "all") else None
        for v in variants:
            for form in ("plain", "bits", "mask", "acc"):
                mask = {"bits": bits, "mask": relu_out}.get(form)
                outs = []
                for a in (None, act):
                    y = base.clone() if form == "acc" else torch.full((M, CIN), 7.0, device=cuda, dtype=torch.bfloat16)
                    CL.launch_hx32(dy, w, None, None, y, g, False, accumulate=form == "acc", variant=v, mask=mask,
                                   active=a)
                    outs.append(y)
                assert torch.equal(outs[0], outs[1]), (name, v, form)
                if name == "zero":
                    assert torch.equal(outs[1], base if form == "acc" else torch.zeros_like(base)), (v, form)
                if ref is not None and form == "plain":
                    err = (outs[0].float() - ref).abs().max().item()
                    assert err <= 2e-2 * ref.abs().max().item() + 1e-2, (name, v, err)
    torch.cuda.synchronize()
    assert RA.LAUNCHES["dgrad"] - n0 == len(PATTERNS) * len(variants) * 4


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_wgrad_row_mask_equals_dense(cuda, geom, cout):
    from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL
    from batchai_retinanet_horovod_coco_amd.ops import conv_wgrad as CW
    from batchai_retinanet_horovod_coco_amd.ops import halo
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    N, shapes = GEOMS[geom]
    M = _rows(N, shapes)
    tab = halo.build_tiles(N, shapes)
    ld = (cout + 63) // 64 * 64
    g = CL.geom_pyramid(N, shapes, CIN, cout)
    gen = torch.Generator(device=cuda).manual_seed(12)
    x = torch.randn(M, CIN, device=cuda, generator=gen).relu().bfloat16().contiguous()
    n0 = RA.LAUNCHES["wgrad"]
    nrun = 0
    for name in PATTERNS:
        sup = _support(name, N, shapes, tab)
        dy = _grad(sup, ld, cout, cuda, seed=1)
        act = _activity(dy, N, shapes).level(0)
        ref = None
        if name in ("random", "all"):
            wz = torch.zeros(cout, CIN, 3, 3, device=cuda, requires_grad=True)
            sum((F.conv2d(xl, wz, padding=1) * dl).sum()
                for xl, dl in zip(_levels(x, N, shapes), _levels(dy[:, :cout], N, shapes))).backward()
            ref = (wz.grad.permute(0, 2, 3, 1), dy[:, :cout].float().sum(0))
        for v in sorted(CW._WGRAD_P8):
            for splits in (None, 1, 3, 7):
                res = []
                for a in (None, act):
                    dw = torch.full((cout, 3, 3, CIN), 3.0, device=cuda)
                    db = torch.full((cout,), 5.0, device=cuda)
                    CW.conv_wgrad(x, dy, g, None, out=dw, variant=v, bias_out=db, splits=splits, rowmask=a)
                    res.append((dw, db))
                nrun += 1
                assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (name, v, splits)
                if name == "zero":
                    assert not res[1][0].any() and not res[1][1].any()
                if ref is not None:
                    for got, want in zip(res[0], ref):
                        err = (got - want).abs().max().item()
                        assert err <= 2e-2 * want.abs().max().item() + 1e-2, (name, v, splits, err)
        # without the fused bias, accumulating into the output
        dws = []
        for a in (None, act):
            dw = torch.full((cout, 3, 3, CIN), 3.0, device=cuda)
            CW.conv_wgrad(x, dy, g, None, out=dw, accumulate=True, variant=24, rowmask=a)
            dws.append(dw)
        nrun += 1
        assert torch.equal(dws[0], dws[1]), name
    torch.cuda.synchronize()
    assert RA.LAUNCHES["wgrad"] - n0 == nrun


def test_training_step_switch_on_equals_off(cuda, monkeypatch):
    """Batch 2 at 256 x 320: the regression tower's backward with the activity chain against the dense one."""
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    from batchai_retinanet_horovod_coco_amd.ops.conv_tuner import TUNER
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer

    torch.manual_seed(0)
    ref_model = models.backbone("resnet18").retinanet(8)
    state = {k: v.clone() for k, v in ref_model.state_dict().items()}
    batch = make_batch(2, 256, 320, num_classes=8, generator=torch.Generator().manual_seed(7))
    # the kernels under test, whatever a race on this shape would pick (the dense run uses the same ones)
    shapes = ((32, 40), (16, 20), (8, 10), (4, 5), (2, 3))
    pins = {TUNER.key("pdgrad", 2, shapes, 256, 256): "hx32_11",
            TUNER.key("pdgrad", 2, shapes, 256, 256) + "|a": "hx32_4",
            TUNER.key("pdgrad", 2, shapes, 256, 256) + "|mb": "hx32_11",
            TUNER.key("pdgrad", 2, shapes, 256, 36) + "|mb": "hx32_6",
            TUNER.key("pwgrad", 2, shapes, 256, 256) + "|s": "hip24"}
    saved = {k: TUNER.table.get(k) for k in pins}
    TUNER.table.update(pins)

    def run(on):
        monkeypatch.setenv("MXR_SPARSE_REG_GRAD", "1" if on else "0")
        n0 = dict(RA.LAUNCHES)
        try:
            model = models.backbone("resnet18").retinanet(8)
            model.load_state_dict(state)
            tr = Trainer(model, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda)
            tr.optimizer.zero_grad()
            b = {k: v.to(cuda) for k, v in batch.items()}
            reg, cls = tr.forward_backward(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            torch.cuda.synchronize()
            grad = tr.flat.grad.clone()
            tr.optimizer.remove_hooks()
            assert model.reg_pad_sink is not None               # the packed heads ran
            return float(reg), float(cls), grad, {k: RA.LAUNCHES[k] - n0[k] for k in n0}
        finally:
            N.set_grad_sinks(None)
            N.set_compute_weights(None)

    try:
        off = run(False)
        on = run(True)
    finally:
        for k, v in saved.items():
            if v is None:
                TUNER.table.pop(k, None)
            else:
                TUNER.table[k] = v
    assert off[3] == {"dgrad": 0, "wgrad": 0}
    assert on[3] == {"dgrad": 5, "wgrad": 4}        # the final's and four tower layers' dX; the four tower dW
    assert on[0] == off[0] and on[1] == off[1]
    assert bool(off[2].any()) and torch.equal(on[2], off[2])
