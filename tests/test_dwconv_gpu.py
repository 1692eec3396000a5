"""``dwconv.hip`` (``mxr_dwconv3x3_fwd / _dgrad / _wgrad``) against the float64 torch expression on the CPU.

Inputs are seeded normal tensors rounded to bf16, so the oracle reads exactly what the kernels read.  Allowances, with
S the same convolution of the absolute values in float64: forward and dgrad (bf16 output of one fp32 sum of at most 9
terms) ``2^-8 |ref| + 2^-20 S``; wgrad (fp32 output, any-order fp32 sum of n = N Ho Wo products) ``2 n 2^-24 S_w``.
Each case prints its worst ratio of error to allowance (``pytest -s``; kept as profiles/dwconv_gpu_tests.log).

The tiles are 8 x 32 (16 from 64 channels on) outputs at stride 1 and 4 x 32 (16) at stride 2, so (2, 17, 33) spans
several tiles per axis at stride 1 only: stride 2 also runs (2, 19, 67), 9 x 33 outputs and 10 x 34 dgrad quads, which
does at every C.
"""
import functools

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import depthwise as D
from batchai_retinanet_horovod_coco_amd.ops import native as N

pytestmark = pytest.mark.gpu

SENTINEL = 12288.0      # exact in bf16
SHAPES = ((1, 2, 3), (3, 5, 7), (2, 17, 33))
CASES = [(s, C, nhw) for s in (1, 2) for C in (8, 24, 136) for nhw in SHAPES + (((2, 19, 67),) if s == 2 else ())]
CASES += [(1, C, (1, 1, 1)) for C in (8, 24, 136)]


def oracle(x, w, dy, stride):
    """(y, dx, dw) of the torch expression in float64."""
    x, w = x.double().requires_grad_(), w.double().requires_grad_()
    y = D.depthwise_conv3x3_torch(x, w, stride)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad


@functools.lru_cache(maxsize=None)
def case(stride, C, nhw):
    """bf16-exact inputs on the CPU, the float64 results, and the same convolutions of the absolute values."""
    n, H, W = nhw
    g = torch.Generator().manual_seed(100 * C + 10 * H + stride)
    x = torch.randn(n, H, W, C, generator=g).bfloat16()
    w = torch.randn(C, 1, 3, 3, generator=g).bfloat16()
    _, _, Ho, Wo = N.dwconv_geometry(H, W, stride)
    dy = torch.randn(n, Ho, Wo, C, generator=g).bfloat16()
    return x, w, dy, oracle(x, w, dy, stride), oracle(x.abs(), w.abs(), dy.abs(), stride)


def guarded(shape, dtype, dev):
    """A tensor of ``shape`` filled with the sentinel, followed by a sentinel row; (tensor, whole buffer)."""
    numel = int(torch.Size(shape).numel())
    buf = torch.full((numel + 64,), SENTINEL, dtype=dtype, device=dev)
    return buf[:numel].view(shape), buf


def run_kernel(kind, stride, C, nhw, dev):
    """One entry point through ctypes on sentinel-filled, sentinel-followed output; returns (out, guard intact)."""
    x, w, dy, _, _ = case(stride, C, nhw)
    n, H, W = nhw
    pt, pl, Ho, Wo = N.dwconv_geometry(H, W, stride)
    xg, dyg, w9 = x.to(dev), dy.to(dev), N.dwconv_taps(w.to(dev))
    geom = (n, H, W, C, stride, pt, pl, Ho, Wo, 1, N._s())
    if kind == "fwd":
        out, buf = guarded((n, Ho, Wo, C), torch.bfloat16, dev)
        rc = N.lib().mxr_dwconv3x3_fwd(N._p(xg), N._p(w9), N._p(out), *geom)
    elif kind == "dgrad":
        out, buf = guarded((n, H, W, C), torch.bfloat16, dev)
        rc = N.lib().mxr_dwconv3x3_dgrad(N._p(dyg), N._p(w9), N._p(out), *geom)
    else:
        out, buf = guarded((9, C), torch.float32, dev)
        work = torch.empty(N.lib().mxr_dwconv_wgrad_work(n, Ho, Wo, C), dtype=torch.float32, device=dev)
        rc = N.lib().mxr_dwconv3x3_wgrad(N._p(dyg), N._p(xg), N._p(out), N._p(work), work.numel(), *geom)
    assert rc == 0
    torch.cuda.synchronize()
    return out, bool((buf[out.numel():] == SENTINEL).all())


@pytest.mark.parametrize("stride,C,nhw", CASES)
@pytest.mark.parametrize("kind", ("fwd", "dgrad", "wgrad"))
def test_kernel_against_float64(cuda, kind, stride, C, nhw):
    _, _, dy, ref, mag = case(stride, C, nhw)
    out, intact = run_kernel(kind, stride, C, nhw, cuda)
    assert intact, "the row after the output was written"
    again, _ = run_kernel(kind, stride, C, nhw, cuda)
    assert torch.equal(out, again), "repeat calls differ"
    out = out.cpu().double()
    if kind == "wgrad":
        r, S = ref[2], mag[2]
        out = out.t().reshape(C, 1, 3, 3)
        allow = 2.0 * (dy.numel() // C) * 2.0 ** -24 * S
    else:
        r, S = (ref[0], mag[0]) if kind == "fwd" else (ref[1], mag[1])
        allow = 2.0 ** -8 * r.abs() + 2.0 ** -20 * S
    err = (out - r).abs()
    ratio = float((err / allow.clamp_min(1e-300)).max())
    print("\n{} stride {} C {} NHW {}: worst |err| / allowance {:.3f}".format(kind, stride, C, nhw, ratio))
    assert bool((err <= allow).all())


def test_dgrad_stride2_zeroes_what_no_window_reads(cuda):
    """(3, 5, 7) at stride 2 with a 1 x 2 dy: the windows read rows 0..2 and columns 0..4; the sentinel-filled dx must
    hold exact zeros elsewhere.  (With the Keras padding the natural Ho x Wo windows reach every row and column of x,
    even or odd, so the unread part is made with the entry point's general Ho / Wo.)"""
    C = 24
    g = torch.Generator().manual_seed(13)
    dy = torch.randn(3, 1, 2, C, generator=g).bfloat16().to(cuda)
    w9 = N.dwconv_taps(torch.randn(C, 1, 3, 3, generator=g).bfloat16().to(cuda))
    dx, buf = guarded((3, 5, 7, C), torch.bfloat16, cuda)
    assert N.lib().mxr_dwconv3x3_dgrad(N._p(dy), N._p(w9), N._p(dx), 3, 5, 7, C, 2, 0, 0, 1, 2, 1, N._s()) == 0
    assert bool((dx[:, 3:] == 0).all()) and bool((dx[:, :, 5:] == 0).all())
    assert bool((dx[:, :3, :5] != SENTINEL).all()) and bool((dx[:, :3, :5] != 0).any())
    assert bool((buf[dx.numel():] == SENTINEL).all())


@pytest.mark.parametrize("dtype,C", ((torch.float32, 8), (torch.bfloat16, 12)))
def test_not_served_falls_back(cuda, dtype, C):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 5, 7, C, generator=g).to(dtype).to(cuda)
    w = torch.randn(C, 1, 3, 3, generator=g).to(dtype).to(cuda)
    w9, y = N.dwconv_taps(w), torch.empty_like(x)
    rc = N.lib().mxr_dwconv3x3_fwd(N._p(x), N._p(w9), N._p(y), 2, 5, 7, C, 1, 1, 1, 5, 7, N._dw_dt(x), N._s())
    assert rc == -1
    with pytest.raises(N.NotServed):
        D.depthwise_conv3x3(x, w, 1, backend="native")
    assert not D.takes_native(x, 1)
    with pytest.warns(UserWarning, match="dwconv.hip does not serve"):
        y = D.depthwise_conv3x3(x, w, 1)
    assert torch.equal(y, D.depthwise_conv3x3_torch(x, w, 1))


@pytest.mark.parametrize("stride", (1, 2))
def test_captured_forward_backward_replays_bit_equal(cuda, stride):
    g = torch.Generator().manual_seed(11)
    n, H, W, C = 2, 17, 33, 24
    w = torch.randn(C, 1, 3, 3, generator=g).bfloat16().to(cuda).requires_grad_()
    xs = [torch.randn(n, H, W, C, generator=g).bfloat16().to(cuda) for _ in range(3)]
    x = xs[0].clone().requires_grad_()

    def step():
        y = N.DepthwiseConv3x3Fn.apply(x, w, stride)
        dx, dw = torch.autograd.grad(y, (x, w), torch.ones_like(y) * 0.5)
        return y, dx, dw

    step()                                       # warm-up outside the capture, on the current stream
    graph = torch.cuda.CUDAGraph()
    # as train/step_graphs.py captures: thread-local mode, the shared capture stream, no stream of the test's own
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = step()
    for new in xs[1:] + xs[1:]:                  # several replays on new input
        with torch.no_grad():
            x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        for a, b in zip(got, step()):
            assert torch.equal(a, b)
    torch.cuda.synchronize()                     # no replay in flight when the graph and its pool go


def test_mobilenet_native_against_float64(cuda):
    """C3..C5 and two depthwise weight gradients of MobileNet(0.25), bf16, 2 x 64 x 96: the native path may deviate
    from the float64 CPU run twice as far as the torch bf16 path does (27 batch-norms on tiny tensors: no bound can be
    derived; both round at the same points and the factor covers another accumulation order)."""
    torch.manual_seed(5)
    ref = MobileNet(0.25).double()
    ref.dw_backend = "torch"
    x = torch.randn(2, 64, 96, 3).bfloat16()

    def run(model, inp):
        outs = model(inp)
        sum(o.float().square().mean() for o in outs).backward()
        return [o.detach().double().cpu() for o in outs] + [model.dw[i].weight.grad.double().cpu() for i in (0, 12)]

    want = run(ref, x.double())
    dev = {}
    for backend in ("torch", "native"):
        m = MobileNet(0.25)
        m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        m.dw_backend = backend
        got = run(m.to(cuda), x.to(cuda))
        assert m.dw_taken == [backend] * 13
        dev[backend] = [float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, want)]
    names = ("C3", "C4", "C5", "dw conv_dw_1", "dw conv_dw_13")
    for name, t, nat in zip(names, dev["torch"], dev["native"]):
        print("\nMobileNet(0.25) {}: max |dev| / max |ref|: torch bf16 {:.3e}, native {:.3e}".format(name, t, nat))
    for name, t, nat in zip(names, dev["torch"], dev["native"]):
        assert nat <= 2.0 * t, name
