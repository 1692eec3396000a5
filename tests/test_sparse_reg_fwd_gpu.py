"""The sparse regression-tower forward (csrc/kernels/row_activity.hip mxr_rows_positive / the un-extended tile rule,
conv_hx32.hip's needed-tiles form):

* the bit kernels against the numpy references (ops/halo.py), ``torch.equal``;
* every hx32 variant's forward walking a needed-tiles list against its own dense launch: equal on the active tiles
  (output and relu bitmask), zero on the others;
* four tower layers and the 64-padded final chained, sparse against dense on the rows each layer's reader needs, and
  the dense chain against an fp32 PyTorch reference (tests/test_proj_fused_gpu.py's tolerance);
* a launch that does not fit the activity's meaning runs dense;
* one small training step in the four combinations of MXR_SPARSE_REG_FWD x MXR_SPARSE_REG_GRAD: the same losses,
  ``torch.equal`` flat gradients, and the launch counters; a forward without the Trainer's request stays dense; a
  captured step replays the eager one."""
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
GROUP = 9
DEPTH = 4


def _rows(N, shapes):
    return N * sum(h * w for h, w in shapes)


def _support(name, N, shapes, tab):
    """bool [M]: the rows that own a positive anchor."""
    M = _rows(N, shapes)
    s = np.zeros(M, dtype=bool)
    if name == "first":
        s[0] = True                      # pixel (0, 0) of image 0, level 0
    elif name == "last":
        s[M - 1] = True                  # the last pixel of the last level of the last image
    elif name in ("edge_out", "edge_in"):
        # one row on either side of a box boundary (a column boundary where the level is split by columns, else a row
        # boundary)
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


def _state(support, cuda):
    """int8 [M * GROUP] anchor states whose positive rows are ``support``: one positive anchor per such row (a
    different one from row to row), ignored (-1) and negative (0) anchors everywhere else."""
    M = len(support)
    st = np.random.default_rng(5).choice(np.array([-1, 0], dtype=np.int8), size=(M, GROUP), p=(0.2, 0.8))
    idx = np.nonzero(support)[0]
    st[idx, idx % GROUP] = 1
    return torch.from_numpy(st.reshape(-1)).to(cuda)


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


def _conv_ref(x, w, b, N, shapes):
    """fp32 3x3 / 'same' conv (+ bias) of the packed bf16 x [M, cin] with w [cout, 3, 3, cin] per level -> [M, cout]."""
    wt = w.float().permute(0, 3, 1, 2)
    return _pack([F.conv2d(l, wt, b.float(), padding=1) for l in _levels(x, N, shapes)])


def _chain(state, N, shapes, depth=DEPTH):
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    ch = RA.FwdChain(depth)
    ch.start(state, GROUP, N, shapes)
    assert ch.acts is not None and ch.current()
    return ch


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_bit_kernels(cuda, geom):
    from batchai_retinanet_horovod_coco_amd.ops import halo
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    N, shapes = GEOMS[geom]
    M = _rows(N, shapes)
    tab = halo.build_tiles(N, shapes)
    tiles, nt = halo.device_tiles(N, shapes, cuda)
    for name in PATTERNS:
        sup = _support(name, N, shapes, tab)
        st = _state(sup, cuda)
        assert np.array_equal(halo.rows_positive(st.cpu().numpy(), GROUP), sup)
        # the mask kernel alone, into a dirty buffer: every word written, tail bits clear
        words = torch.full(((M + 63) // 64,), -1, dtype=torch.int64, device=cuda)
        RA.rows_positive(st, M, GROUP, out=words)
        assert torch.equal(words.cpu(), torch.from_numpy(halo.pack_row_bits(sup).view(np.int64))), name
        # both tile rules from one launch, in an order of the caller's choosing
        masks = torch.stack([words, torch.from_numpy(halo.pack_row_bits(halo.dilate_rows(sup, N, shapes))
                                                     .view(np.int64)).to(cuda)])
        order, count = RA.halo_active_tiles(tiles, nt, masks, which=[1, 0, 0, 1], ext=[0, 0, 1, 1])
        refs = [halo.active_tiles(tab, halo.dilate_rows(sup, N, shapes), ext=0), halo.active_tiles(tab, sup, ext=0),
                halo.active_tiles(tab, sup, ext=1), halo.active_tiles(tab, halo.dilate_rows(sup, N, shapes), ext=1)]
        for i, ref in enumerate(refs):
            cnt = int(count[i].item())
            o = order[i].cpu()
            assert cnt == int(ref.sum()), (name, i)
            assert torch.equal(o[:cnt], torch.from_numpy(np.nonzero(ref)[0].astype(np.int32))), (name, i)
            assert torch.equal(o.sort().values, torch.arange(nt, dtype=torch.int32)), (name, i)
        # the default call form is the extended rule of every mask
        o1, c1 = RA.halo_active_tiles(tiles, nt, masks)
        assert torch.equal(o1[0], order[2]) and torch.equal(o1[1], order[3])
        assert torch.equal(c1, count[2:])
        # the chain: masks M0 .. M4, the lists of the forward (un-extended) and of the backward (extended)
        ch = _chain(st, N, shapes)
        cur = sup
        for k in range(DEPTH + 1):
            for act, ext in ((ch.need(k), 0), (ch.gacts[k], 1)):
                assert torch.equal(act.words.cpu(), torch.from_numpy(halo.pack_row_bits(cur).view(np.int64))), (name, k)
                ref = halo.active_tiles(tab, cur, ext=ext)
                cnt = int(act.count.item())
                assert cnt == int(ref.sum()), (name, k, ext)
                assert torch.equal(act.order.cpu()[:cnt], torch.from_numpy(np.nonzero(ref)[0].astype(np.int32)))
                assert act.need == (ext == 0)
            cur = halo.dilate_rows(cur, N, shapes)


@pytest.mark.parametrize("cout", (256, 64))
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_one_layer_needed_tiles_equal_dense(cuda, geom, cout):
    """cout 256: a tower layer (bias + relu + bitmask); cout 64: the padded final (bias only)."""
    from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL
    from batchai_retinanet_horovod_coco_amd.ops import halo
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    N, shapes = GEOMS[geom]
    M = _rows(N, shapes)
    tab = halo.build_tiles(N, shapes)
    g = CL.geom_pyramid(N, shapes, CIN, cout)
    gen = torch.Generator(device=cuda).manual_seed(21)
    x = torch.randn(M, CIN, device=cuda, generator=gen).relu().bfloat16().contiguous()
    w = (torch.randn(cout, 3, 3, CIN, device=cuda, generator=gen) / (9 * CIN / 2) ** 0.5).bfloat16().contiguous()
    b = torch.randn(cout, device=cuda, generator=gen) * 0.5
    relu = cout == 256
    variants = CL.hx32_variants(g)
    assert set(variants) >= {0, 2, 3, 4, 6, 10, 11, 13, 14} and ((8 in variants and 9 in variants) == (cout == 64))
    n0 = RA.FWD_LAUNCHES["conv"]

    def launch(v, act):
        y = torch.full((M, cout), 7.0, device=cuda, dtype=torch.bfloat16)
        bm = None
        if relu:
            bm = CL.BitMask(shape=(M, cout), device=cuda)
            bm.bits.fill_(0xAA)
        CL.launch_hx32(x, w, b, None, y, g, relu, variant=v, mask=bm, active=act)
        return y, (bm.bits.reshape(M, cout // 8) if relu else None)

    dense = {v: launch(v, None) for v in variants}
    ref = _conv_ref(x, w, b, N, shapes)
    if relu:
        ref = ref.relu()
    for v in variants:
        err = (dense[v][0].float() - ref).abs().max().item()
        assert err <= 2e-2 * ref.abs().max().item() + 1e-2, (v, err)
        if relu:
            assert torch.equal(dense[v][1], CL.BitMask.of(dense[v][0]).bits.reshape(M, cout // 8)), v
    for name in PATTERNS:
        sup = _support(name, N, shapes, tab)
        act = _chain(_state(sup, cuda), N, shapes, depth=0).need(0)
        on = torch.from_numpy(halo.tile_rows(tab, halo.active_tiles(tab, sup, ext=0), M)).to(cuda)
        assert bool(on.any()) == (name != "zero") and (name != "all" or bool(on.all()))
        assert name in ("all", "random") or not bool(on.all())      # (1 % of the rows can reach every tile)
        for v in variants:
            y, bits = launch(v, act)
            yd, bd = dense[v]
            assert torch.equal(y[on], yd[on]), (name, v)
            assert not y[~on].any(), (name, v)
            if relu:
                assert torch.equal(bits[on], bd[on]), (name, v)
                assert not bits[~on].any(), (name, v)
    torch.cuda.synchronize()
    assert RA.FWD_LAUNCHES["conv"] - n0 == len(PATTERNS) * len(variants)


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_five_layers_chained(cuda, geom):
    """4 tower layers (hx32_10 / hx32_11 with bias + relu + bitmask) and the 36-output final through _pad64_pfwd."""
    from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL
    from batchai_retinanet_horovod_coco_amd.ops import halo
    from batchai_retinanet_horovod_coco_amd.ops import native_conv as NC
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    from batchai_retinanet_horovod_coco_amd.ops.conv_tuner import TUNER
    N, shapes = GEOMS[geom]
    M = _rows(N, shapes)
    P = M // N
    tab = halo.build_tiles(N, shapes)
    g = CL.geom_pyramid(N, shapes, CIN, CIN)
    gen = torch.Generator(device=cuda).manual_seed(22)
    x0 = torch.randn(M, CIN, device=cuda, generator=gen).relu().bfloat16().contiguous()
    ws = [(torch.randn(CIN, 3, 3, CIN, device=cuda, generator=gen) / (9 * CIN / 2) ** 0.5).bfloat16().contiguous()
          for _ in range(DEPTH)]
    bs = [torch.randn(CIN, device=cuda, generator=gen) * 0.1 for _ in range(DEPTH)]
    wf = (torch.randn(36, 3, 3, CIN, device=cuda, generator=gen) / (9 * CIN / 2) ** 0.5).bfloat16().contiguous()
    bf = torch.randn(36, device=cuda, generator=gen) * 0.1
    key = TUNER.key("pfwd", N, tuple(shapes), CIN, 64, 0, "pad")
    saved = TUNER.table.get(key)
    TUNER.table[key] = "hx32_9"

    def run(ch):
        outs, x = [], x0
        for i in range(DEPTH):
            y = torch.full((M, CIN), 7.0, device=cuda, dtype=torch.bfloat16)
            bm = CL.BitMask(shape=(M, CIN), device=cuda)
            CL.launch_hx32(x, ws[i], bs[i], None, y, g, True, variant=(10, 11)[i % 2], mask=bm,
                           active=None if ch is None else ch.need(DEPTH - i))
            outs.append(y)
            x = y
        outs.append(NC._pad64_pfwd(x.reshape(N, P, CIN), wf, bf, shapes, False,
                                   need=None if ch is None else ch.need(0)).reshape(M, 36))
        return outs

    try:
        dense = run(None)
        x = x0
        for i in range(DEPTH + 1):         # the yardstick itself, layer by layer
            ref = _conv_ref(x, wf if i == DEPTH else ws[i], bf if i == DEPTH else bs[i], N, shapes)
            ref = ref if i == DEPTH else ref.relu()
            err = (dense[i].float() - ref).abs().max().item()
            assert err <= 2e-2 * ref.abs().max().item() + 1e-2, (i, err)
            x = dense[i]
        for name in PATTERNS:
            sup = _support(name, N, shapes, tab)
            n0 = RA.FWD_LAUNCHES["conv"]
            sparse = run(_chain(_state(sup, cuda), N, shapes))
            assert RA.FWD_LAUNCHES["conv"] - n0 == DEPTH + 1
            mk = [sup]
            for _ in range(DEPTH):
                mk.append(halo.dilate_rows(mk[-1], N, shapes))
            for i in range(DEPTH + 1):
                rows = torch.from_numpy(mk[DEPTH - i]).to(cuda)     # layer i is DEPTH - i below the final
                assert torch.equal(sparse[i][rows], dense[i][rows]), (name, i)
                assert bool(torch.isfinite(sparse[i].float()).all()), (name, i)
            if name == "all":
                assert all(torch.equal(a, b) for a, b in zip(sparse, dense))
            if name == "zero":
                assert not any(bool(a.any()) for a in sparse)
    finally:
        if saved is None:
            TUNER.table.pop(key, None)
        else:
            TUNER.table[key] = saved


def test_a_mismatch_falls_back_to_dense(cuda):
    from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL
    from batchai_retinanet_horovod_coco_amd.ops import halo
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    N, shapes = GEOMS["ragged"]
    M = _rows(N, shapes)
    tab = halo.build_tiles(N, shapes)
    g = CL.geom_pyramid(N, shapes, CIN, CIN)
    gen = torch.Generator(device=cuda).manual_seed(23)
    x = torch.randn(M, CIN, device=cuda, generator=gen).bfloat16().contiguous()
    w = (torch.randn(CIN, 3, 3, CIN, device=cuda, generator=gen) / 48).bfloat16().contiguous()
    b = torch.randn(CIN, device=cuda, generator=gen)
    base = torch.randn(M, CIN, device=cuda, generator=gen).bfloat16()
    ch = _chain(_state(_support("first", N, shapes, tab), cuda), N, shapes, depth=0)
    n0 = (dict(RA.LAUNCHES), dict(RA.FWD_LAUNCHES))

    def launch(act, bias, accumulate):
        y = base.clone()
        CL.launch_hx32(x, w, bias, None, y, g, False, accumulate=accumulate, variant=10, active=act)
        return y

    # a zero-input activity with a bias; a needed-tiles activity with an accumulate
    assert torch.equal(launch(ch.gacts[0], b, False), launch(None, b, False))
    assert torch.equal(launch(ch.need(0), None, True), launch(None, None, True))
    # (and a needed-tiles activity inside a `using` block reaches the launch that fits it)
    with RA.using(ch.need(0)):
        y = launch(None, b, False)
    assert not y[M // 2:].any() and bool(y[0].any())
    torch.cuda.synchronize()
    assert RA.LAUNCHES == n0[0] and RA.FWD_LAUNCHES["conv"] - n0[1]["conv"] == 1


SHAPES_STEP = ((32, 40), (16, 20), (8, 10), (4, 5), (2, 3))      # batch 2 at 256 x 320


def _pins():
    from batchai_retinanet_horovod_coco_amd.ops.conv_tuner import TUNER
    s = SHAPES_STEP
    # the kernels under test, whatever a race on this shape would pick (the dense runs use the same ones)
    return {TUNER.key("pfwd", 2, s, 256, 256, 1) + "|eb": "hx32_10",
            TUNER.key("pfwd", 2, s, 256, 36, 0): "pad64",
            TUNER.key("pfwd", 2, s, 256, 64, 0, "pad"): "hx32_9",
            TUNER.key("pdgrad", 2, s, 256, 256): "hx32_11",
            TUNER.key("pdgrad", 2, s, 256, 256) + "|a": "hx32_4",
            TUNER.key("pdgrad", 2, s, 256, 256) + "|mb": "hx32_11",
            TUNER.key("pdgrad", 2, s, 256, 36) + "|mb": "hx32_6",
            TUNER.key("pwgrad", 2, s, 256, 256) + "|s": "hip24"}


class _Pinned:
    def __enter__(self):
        from batchai_retinanet_horovod_coco_amd.ops.conv_tuner import TUNER
        pins = _pins()
        self.saved = {k: TUNER.table.get(k) for k in pins}
        TUNER.table.update(pins)

    def __exit__(self, *exc):
        from batchai_retinanet_horovod_coco_amd.ops.conv_tuner import TUNER
        for k, v in self.saved.items():
            if v is None:
                TUNER.table.pop(k, None)
            else:
                TUNER.table[k] = v
        return False


def _counters():
    from batchai_retinanet_horovod_coco_amd.ops import row_activity as RA
    return {"conv": RA.FWD_LAUNCHES["conv"], "mask_fwd": RA.MASK_LAUNCHES["fwd"], "mask_bwd": RA.MASK_LAUNCHES["bwd"],
            "dgrad": RA.LAUNCHES["dgrad"], "wgrad": RA.LAUNCHES["wgrad"]}


@pytest.fixture(scope="module")
def step_setup():
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in models.backbone("resnet18").retinanet(8).state_dict().items()}
    batch = make_batch(2, 256, 320, num_classes=8, generator=torch.Generator().manual_seed(7))
    return state, batch


@pytest.mark.parametrize("regression_loss", ("smooth_l1", "giou"))
def test_training_step_four_switch_combinations(cuda, monkeypatch, step_setup, regression_loss):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    state, batch = step_setup

    def run(fwd, grad):
        monkeypatch.setenv("MXR_SPARSE_REG_FWD", "1" if fwd else "0")
        monkeypatch.setenv("MXR_SPARSE_REG_GRAD", "1" if grad else "0")
        n0 = _counters()
        try:
            model = models.backbone("resnet18").retinanet(8)
            model.load_state_dict(state)
            tr = Trainer(model, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda,
                         regression_loss=regression_loss)
            tr.optimizer.zero_grad()
            b = {k: v.to(cuda) for k, v in batch.items()}
            reg, cls = tr.forward_backward(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            torch.cuda.synchronize()
            grad_ = tr.flat.grad.clone()
            tr.optimizer.remove_hooks()
            assert model.reg_pad_sink is not None               # the packed heads ran
            assert getattr(model, "positive_request", None) is None     # cleared with the forward
            n1 = _counters()
            return float(reg), float(cls), grad_, {k: n1[k] - n0[k] for k in n0}
        finally:
            N.set_grad_sinks(None)
            N.set_compute_weights(None)

    with _Pinned():
        res = {(f, g): run(f, g) for f in (False, True) for g in (False, True)}
    ref = res[(False, False)]
    assert bool(ref[2].any()) and ref[0] > 0 and ref[1] > 0
    for (f, g), r in res.items():
        assert r[0] == ref[0] and r[1] == ref[1], (f, g)
        assert torch.equal(r[2], ref[2]), (f, g)
        want = {"conv": 5 if f else 0, "mask_fwd": 3 if f else 0, "mask_bwd": 3 if (g and not f) else 0,
                "dgrad": 5 if g else 0, "wgrad": 4 if g else 0}
        assert r[3] == want, (f, g, r[3])


def test_no_request_no_sparsity(cuda, monkeypatch, step_setup):
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native as N
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    state, batch = step_setup

    def run(fwd, grad_mode):
        monkeypatch.setenv("MXR_SPARSE_REG_FWD", "1" if fwd else "0")
        n0 = _counters()
        try:
            model = models.backbone("resnet18").retinanet(8)
            model.load_state_dict(state)
            tr = Trainer(model, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda)
            x = batch["images"].to(cuda).to(torch.bfloat16)
            with torch.set_grad_enabled(grad_mode):
                reg = tr.model(x)["regression"].detach().clone()        # a direct call: no Trainer request
            torch.cuda.synchronize()
            tr.optimizer.remove_hooks()
            n1 = _counters()
            return reg, {k: n1[k] - n0[k] for k in n0}
        finally:
            N.set_grad_sinks(None)
            N.set_compute_weights(None)

    with _Pinned():
        for grad_mode in (False, True):
            on, off = run(True, grad_mode), run(False, grad_mode)
            assert torch.equal(on[0], off[0]) and bool(on[0].any())
            assert on[1]["conv"] == 0 and on[1]["mask_fwd"] == 0 and off[1]["conv"] == 0


def test_captured_step_equals_eager(cuda, monkeypatch, step_setup):
    """One graph_step replay against the eager step, the sparse forward inside the capture."""
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.ops import native
    from batchai_retinanet_horovod_coco_amd.parallel import ops
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer
    state, batch = step_setup
    monkeypatch.setenv("MXR_SPARSE_REG_FWD", "1")
    monkeypatch.setenv("MXR_SPARSE_REG_GRAD", "1")
    b = {k: v.to(cuda) for k, v in batch.items()}

    def run(graphed):
        native.set_grad_sinks(None)
        native.set_compute_weights(None)
        model = models.backbone("resnet18").retinanet(8)
        model.load_state_dict(state)
        tr = Trainer(model, lr=1e-4, clipnorm=0.001, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda)
        try:
            n0 = _counters()
            if graphed:
                step = tr.graph_step(b["images"], b["gt"], b["gt_count"], b["image_hw"], warmup=2)
            else:
                step = tr.train_on_batch
                for _ in range(2):
                    step(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            n1 = _counters()
            loss = step(b["images"], b["gt"], b["gt_count"], b["image_hw"])["loss"].clone()
            torch.cuda.synchronize()
            return loss, tr.flat.data.clone(), {k: n1[k] - n0[k] for k in n0}
        finally:
            if getattr(tr.optimizer, "native", None) is not None:
                ops.set_native_comm(None)
                tr.optimizer.native.close()
            tr.optimizer.remove_hooks()
            native.set_grad_sinks(None)
            native.set_compute_weights(None)

    with _Pinned():
        run(False)                         # first sight: the conv tuner races here, not below
        eager = run(False)
        graph = run(True)
    # two warm-up steps, and for the graph the captured one: each with the sparse forward and no backward mask kernels
    assert eager[2]["conv"] == 10 and graph[2]["conv"] == 15 and graph[2]["mask_bwd"] == 0
    assert torch.equal(eager[0], graph[0]), (eager[0].item(), graph[0].item())
    assert torch.equal(eager[1], graph[1])
