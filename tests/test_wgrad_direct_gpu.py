"""The slab-free ("direct") weight gradient of conv_wgrad_pipe.hip (``conv_wgrad`` variants 30 / 31): one split over the
whole pixel range, the epilogue writes ``out[co, k] = (accumulate ? out : 0) + scale[co] * acc`` itself -- no fp32
slabs, no reduce launch.  Checked against the fp32 weight gradient of the bf16-rounded operands (the bound of
``test_kernels_gpu.py::test_wgrad_variants``) and against the slab form of the same tile at one split, which runs the
same MFMA sequence: only the epilogue's multiply-add may round differently (one fp32 rounding, fused vs separate)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (n, H, W, cin, cout, k, stride, pad)
CASES = {
    "short_ring": (1, 7, 9, 64, 64, 3, 1, "same"),         # 2 sub-stages < ring depth; K = 576: partial k tile
    "two_pixels": (1, 1, 2, 256, 256, 1, 1, "valid"),      # M = 2
    "padded_dy": (1, 13, 19, 128, 36, 3, 1, "same"),       # dY padded to 40 columns, partial co tile
    "strided": (2, 21, 34, 256, 128, 1, 2, "valid"),       # strided gather, image carry
    "stage5": (1, 25, 42, 512, 512, 3, 1, "same"),
    "pyramid": (1, [(10, 17), (5, 9), (3, 5), (2, 3), (1, 2)], None, 256, 72, 3, 1, "same"),    # level carries
}
VARIANTS = [30, 31]
_DATA = {}


def _ref_level(x, dy, k, s, p):
    """fp64 dW (cout, k, k, cin) of one NHWC level from its im2col."""
    n, H, W, cin = x.shape
    cout = dy.shape[-1]
    cols = F.unfold(x.permute(0, 3, 1, 2).double(), k, padding=p, stride=s)            # (n, cin * k * k, L)
    d = dy.reshape(n, -1, cout).double()
    dw = torch.einsum("nlo,nkl->ok", d, cols)
    return dw.view(cout, cin, k, k).permute(0, 2, 3, 1)


def _data(name, cuda):
    """Operands, geometry and the fp32 reference of a case: built once, shared, never modified."""
    if name in _DATA:
        return _DATA[name]
    from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL
    n, H, W, cin, cout, k, s, pm = CASES[name]
    gen = torch.Generator(device=cuda).manual_seed(len(name) * 7 + cin)
    p = 1 if pm == "same" else 0
    if isinstance(H, list):
        shapes = H
        xs = [torch.randn(n, h, w, cin, device=cuda, generator=gen).bfloat16() for h, w in shapes]
        dys = [torch.randn(n, h, w, cout, device=cuda, generator=gen).bfloat16() for h, w in shapes]
        x = torch.cat([t.reshape(n, -1, cin) for t in xs], 1).contiguous()
        dy = torch.cat([t.reshape(n, -1, cout) for t in dys], 1).contiguous()
        g = CL.geom_pyramid(n, shapes, cin, cout)
        ref = sum(_ref_level(a, b, k, s, p) for a, b in zip(xs, dys))
    else:
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        x = torch.randn(n, H, W, cin, device=cuda, generator=gen).bfloat16()
        dy = torch.randn(n, Ho, Wo, cout, device=cuda, generator=gen).bfloat16()
        g = CL.geom_single(n, H, W, Ho, Wo, k, s, (p, p, p, p), cin, cout)
        ref = _ref_level(x, dy, k, s, p)
    scale = torch.rand(cout, device=cuda, generator=gen) + 0.5
    base = torch.randn(cout, k, k, cin, device=cuda, generator=gen)
    _DATA[name] = (x, dy, g, scale, base, ref.float())
    return _DATA[name]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_direct_wgrad(cuda, name, variant):
    from batchai_retinanet_horovod_coco_amd.ops import conv_wgrad as CW
    x, dy, g, scale, base, ref = _data(name, cuda)
    slab_variant = CW._WGRAD_DIRECT[variant][2]
    assert CW._WGRAD_PIPE_TILE[slab_variant] == CW._WGRAD_DIRECT[variant][0]
    peak = ref.abs().max().item()

    # scaled, written
    dw = CW.conv_wgrad(x, dy, g, scale, variant=variant)
    want = ref * scale.view(-1, 1, 1, 1)
    err = (dw - want).abs().max().item() / want.abs().max().item()
    slab = CW.conv_wgrad(x, dy, g, scale, variant=slab_variant, splits=1)
    d_slab = (dw - slab).abs().max().item()
    print("%s hip%d: rel err %.3e, vs slab form at one split %.3e (of max |ref| %.3e)" % (name, variant, err, d_slab, peak))
    assert err < 1e-2
    assert d_slab <= 1e-6 * want.abs().max().item()
    assert torch.equal(dw, CW.conv_wgrad(x, dy, g, scale, variant=variant))        # deterministic

    # unscaled, accumulated onto a random gradient
    out = base.clone()
    CW.conv_wgrad(x, dy, g, None, out=out, accumulate=True, variant=variant)
    out_slab = base.clone()
    CW.conv_wgrad(x, dy, g, None, out=out_slab, accumulate=True, variant=slab_variant, splits=1)
    err = (out - (base + ref)).abs().max().item() / peak
    d_slab = (out - out_slab).abs().max().item()
    print("%s hip%d accumulate: rel err %.3e, vs slab form %.3e" % (name, variant, err, d_slab))
    assert err < 1e-2
    assert d_slab <= 1e-6 * peak
    again = base.clone()
    CW.conv_wgrad(x, dy, g, None, out=again, accumulate=True, variant=variant)
    assert torch.equal(out, again)


def test_direct_candidates_join_the_race_only_where_covered(cuda):
    from batchai_retinanet_horovod_coco_amd.ops import conv_wgrad as CW
    x, dy, g, scale, _, _ = _data("stage5", cuda)
    assert CW.direct_covers(g)
    names = set(CW.wgrad_candidates(x, dy, g, scale))
    assert {"hip30", "hip31"} <= names
    sink = torch.zeros(g.cout * 9 * g.cin, device=cuda)
    def make(sink, only=None):
        return CW.wgrad_candidates(x, dy, g, scale, only=only, sink=sink, lib_fn=lambda: None)
    assert {"hip30", "hip31"} <= set(make(sink))
    assert list(make(sink, "hip30")) == ["hip30"]
    for other in ("short_ring", "pyramid"):        # too few tiles / a packed pyramid: not raced
        x, dy, g, scale, _, _ = _data(other, cuda)
        assert not CW.direct_covers(g)
        assert not {"hip30", "hip31"} & set(CW.wgrad_candidates(x, dy, g, scale))
