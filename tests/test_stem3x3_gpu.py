"""``stem3x3.hip`` (``mxr_stem3_fwd / _wgrad``) against the float64 torch expression on the CPU.

Inputs are seeded normal tensors rounded to bf16, weights included, so the oracle reads exactly what the kernels read.
Allowances, with S the same expression on the absolute values in float64: forward (bf16 output of one fp32 sum of 27
exact products in any order) ``2^-8 |ref| + 2 * 27 * 2^-24 S``; weight gradient (fp32 output, any-order fp32 sum of
M = N Ho Wo products) ``2 M 2^-24 S``.  Each case prints its worst ratio of error to allowance (``pytest -s``; kept as
profiles/stem3x3_gpu_tests.log).

Boundaries of the design (tiles of 4 output rows x 64 output columns, one per workgroup and step; grids of at most 2048
(forward) and 1024 (weight gradient) workgroups), and the cases beyond the issue's grid that cross them at small M:
* a second and third column tile, the last of one pixel (odd W) or with the pad column in it (even W): (1, 5, 131),
  (1, 4, 258);
* more than one weight-gradient partial: every case with more than one tile, (2, 37, 70) has 10;
* a second (and third) tile per workgroup, on both grids: (2060, 5, 6), one tile per image;
* the last partial word of a row, and rows that alternate between the two 4-byte alignments: odd W, (2, 8, 13);
* an image at a storage offset of one element (``data_ptr() % 4 == 2``) is SERVED, by the entry point and by
  ``stem3_served`` alike: rows are fetched as aligned words whatever the base, see ``test_odd_offset_view``.
"""
import functools

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops import stem3x3 as S3

pytestmark = pytest.mark.gpu

SENTINEL = 12288.0      # exact in bf16
SIZES = ((1, 2, 2), (1, 3, 3), (2, 9, 14), (2, 8, 13), (2, 37, 70))
CASES = [(co, nhw) for co in (8, 16, 24, 32) for nhw in SIZES]
CASES += [(16, (1, 5, 131)), (24, (1, 4, 258)), (8, (2060, 5, 6)), (32, (2060, 5, 6))]


def oracle(x, w, dy):
    """(y, dw) of the torch expression in float64."""
    w = w.double().requires_grad_()
    y = S3.stem_conv3x3_torch(x.double(), w)
    y.backward(dy.double())
    return y.detach(), w.grad


@functools.lru_cache(maxsize=None)
def case(co, nhw):
    """bf16-exact inputs on the CPU, the float64 results, and the same expressions on the absolute values."""
    g = torch.Generator().manual_seed(100 * co + nhw[1])
    x = torch.randn(*nhw, 3, generator=g).bfloat16()
    w = torch.randn(co, 3, 3, 3, generator=g).bfloat16()
    n, ho, wo = nhw[0], (nhw[1] - 2) // 2 + 1, (nhw[2] - 2) // 2 + 1
    dy = torch.randn(n, ho, wo, co, generator=g).bfloat16()
    return x, w, dy, oracle(x, w, dy), oracle(x.abs(), w.abs(), dy.abs())


def guarded(shape, dtype, dev):
    """A tensor of ``shape`` filled with the sentinel, followed by a sentinel run; (tensor, whole buffer)."""
    numel = int(torch.Size(shape).numel())
    buf = torch.full((numel + 64,), SENTINEL, dtype=dtype, device=dev)
    return buf[:numel].view(shape), buf


def run_kernel(kind, co, nhw, dev, offset=0):
    """One entry point through ctypes on sentinel-filled, sentinel-followed output, the image ``offset`` elements into
    its buffer; returns (out, guard intact)."""
    x, w, dy, _, _ = case(co, nhw)
    xg = torch.zeros(x.numel() + offset, dtype=torch.bfloat16, device=dev)[offset:].view(x.shape).copy_(x)
    assert xg.data_ptr() % 4 == 2 * offset
    n, H, W = nhw
    if kind == "fwd":
        out, buf = guarded(tuple(dy.shape), torch.bfloat16, dev)
        rc = N.lib().mxr_stem3_fwd(N._p(xg), N._p(N.stem3_weight(w.to(dev))), N._p(out), n, H, W, co, 1, 0, N._s())
    else:
        dyg = dy.to(dev)
        out, buf = guarded((co, 3, 3, 3), torch.float32, dev)
        nwork = N.lib().mxr_stem3_wgrad_work(n, dy.shape[1], dy.shape[2], co)
        tiles = n * ((dy.shape[1] + 3) // 4) * ((dy.shape[2] + 63) // 64)
        assert nwork == min(tiles, 1024) * co * 32
        work = torch.empty(nwork, dtype=torch.float32, device=dev)
        rc = N.lib().mxr_stem3_wgrad(N._p(dyg), N._p(xg), N._p(out), N._p(work), nwork, n, H, W, co, 1, N._s())
    assert rc == 0
    torch.cuda.synchronize()
    return out, bool((buf[out.numel():] == SENTINEL).all())


@pytest.mark.parametrize("co,nhw", CASES)
@pytest.mark.parametrize("kind", ("fwd", "wgrad"))
def test_kernel_against_float64(cuda, kind, co, nhw):
    _, _, dy, ref, mag = case(co, nhw)
    out, intact = run_kernel(kind, co, nhw, cuda)
    assert intact, "the run after the output was written"
    assert not bool((out == SENTINEL).any()), "an element of the output was not written"
    again, _ = run_kernel(kind, co, nhw, cuda)
    assert torch.equal(out, again), "repeat calls differ"
    i = ("fwd", "wgrad").index(kind)
    r, S = ref[i], mag[i]
    if kind == "wgrad":
        allow = 2.0 * (dy.numel() // co) * 2.0 ** -24 * S
    else:
        allow = 2.0 ** -8 * r.abs() + 2.0 * 27 * 2.0 ** -24 * S
    err = (out.cpu().double() - r).abs()
    ratio = float((err / allow.clamp_min(1e-300)).max())
    print("\n{} Co {} NHW {}: worst |err| / allowance {:.3f}".format(kind, co, nhw, ratio))
    assert bool((err <= allow).all())


@pytest.mark.parametrize("kind", ("fwd", "wgrad"))
@pytest.mark.parametrize("co,nhw", ((24, (2, 8, 13)), (16, (2, 9, 14))))
def test_odd_offset_view(cuda, kind, co, nhw):
    """Served: the same bits as the aligned image gives."""
    view = torch.zeros(nhw[0] * nhw[1] * nhw[2] * 3 + 1, dtype=torch.bfloat16, device=cuda)[1:].view(*nhw, 3)
    assert view.data_ptr() % 4 == 2 and N.stem3_served(view, co)
    out, intact = run_kernel(kind, co, nhw, cuda, offset=1)
    assert intact
    assert torch.equal(out, run_kernel(kind, co, nhw, cuda)[0])


def test_wgrad_refuses_short_work(cuda):
    x = torch.zeros(2, 37, 70, 3, dtype=torch.bfloat16, device=cuda)
    dy = torch.zeros(2, 18, 35, 8, dtype=torch.bfloat16, device=cuda)
    dw = torch.zeros(8, 3, 3, 3, dtype=torch.float32, device=cuda)
    nwork = N.lib().mxr_stem3_wgrad_work(2, 18, 35, 8)
    work = torch.zeros(nwork, dtype=torch.float32, device=cuda)
    assert N.lib().mxr_stem3_wgrad(N._p(dy), N._p(x), N._p(dw), N._p(work), nwork - 1, 2, 37, 70, 8, 1, N._s()) == -2


@pytest.mark.parametrize("dtype,co,H,grad", ((torch.float32, 8, 6, False), (torch.bfloat16, 12, 6, False),
                                             (torch.bfloat16, 40, 6, False), (torch.bfloat16, 8, 1, False),
                                             (torch.bfloat16, 8, 6, True)))
def test_not_served_falls_back(cuda, dtype, co, H, grad):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, H, 7, 3, generator=g).to(dtype).to(cuda).requires_grad_(grad)
    w = torch.randn(co, 3, 3, 3, generator=g).to(cuda)
    wpk = torch.zeros(32, 32, dtype=torch.bfloat16, device=cuda)
    y = torch.empty(2 * 3 * 3 * co, dtype=dtype, device=cuda)
    assert N.lib().mxr_stem3_fwd(N._p(x), N._p(wpk), N._p(y), 2, H, 7, co, N._dw_dt(x), int(grad), N._s()) == -1
    with pytest.raises(N.NotServed):
        S3.stem_conv3x3(x, w, backend="native")
    assert not S3.takes_native(x, co)
    assert not S3.takes_native(x, co, "native")
    if dtype != torch.float32:
        return      # torch ops on odd-channel bf16 channels-last views have segfaulted inside torch (README)
    with pytest.warns(UserWarning, match="stem3x3.hip does not serve"):
        y = S3.stem_conv3x3(x, w)
    assert torch.equal(y, S3.stem_conv3x3_torch(x, w))


def test_captured_forward_backward_replays_bit_equal(cuda):
    g = torch.Generator().manual_seed(11)
    w = torch.randn(24, 3, 3, 3, generator=g).to(cuda).requires_grad_()
    xs = [torch.randn(2, 37, 70, 3, generator=g).bfloat16().to(cuda) for _ in range(3)]
    x = xs[0].clone()

    def step():
        y = N.Stem3x3Fn.apply(x, w)
        dw, = torch.autograd.grad(y, (w,), torch.ones_like(y) * 0.5)
        return y, dw

    step()                                       # warm-up outside the capture, on the current stream
    graph = torch.cuda.CUDAGraph()
    # as train/step_graphs.py captures: thread-local mode, the shared capture stream, no stream of the test's own
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = step()
    for new in xs[1:] + xs[1:]:                  # several replays on new input
        x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        for a, b in zip(got, step()):
            assert torch.equal(a, b)
    torch.cuda.synchronize()                     # no replay in flight when the graph and its pool go


def test_mobilenet_native_against_float64(cuda):
    """C3..C5 and the stem's weight gradient of MobileNet(0.25), bf16, 2 x 64 x 96: with the native stem, C3 and C4 may
    deviate from the float64 CPU run twice as far as with the torch bf16 stem (the pointwise model test's rule: 27
    batch-norms on tiny tensors, no bound can be derived; both round at the same points and the factor covers another
    accumulation order).  C5 and the weight gradient are printed only: the existing model tests record that the torch
    bf16 path itself is about 1 x max |ref| away there."""
    torch.manual_seed(5)
    ref = MobileNet(0.25).double()
    x = torch.randn(2, 64, 96, 3).bfloat16()

    def run(model, inp):
        outs = model(inp)
        sum(o.float().square().mean() for o in outs).backward()
        return [o.detach().double().cpu() for o in outs] + [model.conv1.weight.grad.double().cpu()]

    want = run(ref, x.double())
    assert ref.stem_taken == "torch"
    dev = {}
    for backend in ("torch", "native"):
        m = MobileNet(0.25)
        m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        m.stem_backend = backend
        got = run(m.to(cuda), x.to(cuda))
        assert m.stem_taken == backend
        assert [g.shape for g in got] == [r.shape for r in want]
        dev[backend] = [float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, want)]
    names = ("C3", "C4", "C5", "dw conv1")
    for name, t, nat in zip(names, dev["torch"], dev["native"]):
        print("\nMobileNet(0.25) {}: max |dev| / max |ref|: torch bf16 {:.3e}, native {:.3e}".format(name, t, nat))
    for name, t, nat in zip(names[:2], dev["torch"], dev["native"]):
        assert nat <= 2.0 * t, name
