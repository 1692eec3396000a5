"""``pwconv.hip`` (``mxr_pwconv_fwd / _dgrad / _wgrad``) against the float64 torch expression on the CPU.

Inputs are seeded normal tensors rounded to bf16, so the oracle reads exactly what the kernels read.  Allowances, with
S the same product of the absolute values in float64: forward and dgrad (bf16 output of one fp32 sum of K = Ci or Co
exact products in any order) ``2^-8 |ref| + 2 K 2^-24 S``; wgrad (fp32 output, any-order fp32 sum of M products)
``2 M 2^-24 S``.  Each case prints its worst ratio of error to allowance (``pytest -s``; kept as
profiles/pwconv_gpu_tests.log).

Regime boundaries of the design, and the cases beyond the issue's grid that cross them at small M:
* forward / dgrad, K <= 128 (weight resident in LDS) against K > 128 (128-k stages): (136, 24) and (40, 136) cross it
  with two stages; (264, 16) and (16, 264) at M = 35 run three stages, the last of one 8-wide vector, and three
  128-wide column blocks;
* column tiles of 32 / 64 / 128 channels (forward, dgrad and both sides of wgrad): crossed by the issue's pairs;
* a workgroup that walks a second row tile without laying the weight again (more than 1024 row tiles of 256), and a
  wgrad split of more than one 64-row stage (M > 65536): (8, 8) at M = 262179; the wgrad split is 64 rows below that,
  so M = 1122 already runs 18 splits.
"""
import functools

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops import pointwise as P

pytestmark = pytest.mark.gpu

SENTINEL = 12288.0      # exact in bf16
PAIRS = ((8, 8), (24, 40), (40, 136), (136, 24), (64, 128))
CASES = [(ci, co, nhw) for ci, co in PAIRS for nhw in ((1, 1, 1), (1, 5, 7), (2, 17, 33))]
CASES += [(264, 16, (1, 5, 7)), (16, 264, (1, 5, 7)), (8, 8, (1, 1, 262179))]


def oracle(x, w, dy):
    """(y, dx, dw) of the torch expression in float64."""
    x, w = x.double().requires_grad_(), w.double().requires_grad_()
    y = P.pointwise_conv_torch(x, w)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad


@functools.lru_cache(maxsize=None)
def case(ci, co, nhw):
    """bf16-exact inputs on the CPU, the float64 results, and the same products of the absolute values."""
    g = torch.Generator().manual_seed(1000 * ci + co)
    x = torch.randn(*nhw, ci, generator=g).bfloat16()
    w = torch.randn(co, ci, 1, 1, generator=g).bfloat16()
    dy = torch.randn(*nhw, co, generator=g).bfloat16()
    return x, w, dy, oracle(x, w, dy), oracle(x.abs(), w.abs(), dy.abs())


def guarded(shape, dtype, dev):
    """A tensor of ``shape`` filled with the sentinel, followed by a sentinel run; (tensor, whole buffer)."""
    numel = int(torch.Size(shape).numel())
    buf = torch.full((numel + 64,), SENTINEL, dtype=dtype, device=dev)
    return buf[:numel].view(shape), buf


def run_kernel(kind, ci, co, nhw, dev):
    """One entry point through ctypes on sentinel-filled, sentinel-followed output; returns (out, guard intact)."""
    x, w, dy, _, _ = case(ci, co, nhw)
    m = x.numel() // ci
    xg, dyg, w2 = x.to(dev), dy.to(dev), N.pwconv_weight(w.to(dev))
    if kind == "fwd":
        out, buf = guarded(nhw + (co,), torch.bfloat16, dev)
        rc = N.lib().mxr_pwconv_fwd(N._p(xg), N._p(w2), N._p(out), m, ci, co, 1, N._s())
    elif kind == "dgrad":
        out, buf = guarded(nhw + (ci,), torch.bfloat16, dev)
        wt = torch.empty(ci, co, dtype=torch.bfloat16, device=dev)
        rc = N.lib().mxr_pwconv_dgrad(N._p(dyg), N._p(w2), N._p(wt), N._p(out), m, ci, co, 1, N._s())
    else:
        out, buf = guarded((co, ci, 1, 1), torch.float32, dev)
        nwork = N.lib().mxr_pwconv_wgrad_work(m, ci, co)
        assert nwork >= co * ci * (2 if m >= 1122 else 1)
        work = torch.empty(nwork, dtype=torch.float32, device=dev)
        rc = N.lib().mxr_pwconv_wgrad(N._p(dyg), N._p(xg), N._p(out), N._p(work), nwork, m, ci, co, 1, N._s())
    assert rc == 0
    torch.cuda.synchronize()
    return out, bool((buf[out.numel():] == SENTINEL).all())


@pytest.mark.parametrize("ci,co,nhw", CASES)
@pytest.mark.parametrize("kind", ("fwd", "dgrad", "wgrad"))
def test_kernel_against_float64(cuda, kind, ci, co, nhw):
    x, _, _, ref, mag = case(ci, co, nhw)
    out, intact = run_kernel(kind, ci, co, nhw, cuda)
    assert intact, "the run after the output was written"
    again, _ = run_kernel(kind, ci, co, nhw, cuda)
    assert torch.equal(out, again), "repeat calls differ"
    i = ("fwd", "dgrad", "wgrad").index(kind)
    r, S = ref[i], mag[i]
    if kind == "wgrad":
        allow = 2.0 * (x.numel() // ci) * 2.0 ** -24 * S
    else:
        allow = 2.0 ** -8 * r.abs() + 2.0 * (ci if kind == "fwd" else co) * 2.0 ** -24 * S
    err = (out.cpu().double() - r).abs()
    ratio = float((err / allow.clamp_min(1e-300)).max())
    print("\n{} Ci {} Co {} NHW {}: worst |err| / allowance {:.3f}".format(kind, ci, co, nhw, ratio))
    assert bool((err <= allow).all())


def test_wgrad_refuses_short_work(cuda):
    x = torch.zeros(1122, 8, dtype=torch.bfloat16, device=cuda)
    dw = torch.zeros(8, 8, dtype=torch.float32, device=cuda)
    nwork = N.lib().mxr_pwconv_wgrad_work(1122, 8, 8)
    work = torch.zeros(nwork, dtype=torch.float32, device=cuda)
    assert N.lib().mxr_pwconv_wgrad(N._p(x), N._p(x), N._p(dw), N._p(work), nwork - 1, 1122, 8, 8, 1, N._s()) == -2


@pytest.mark.parametrize("dtype,ci,co", ((torch.float32, 8, 8), (torch.bfloat16, 12, 8), (torch.bfloat16, 8, 12)))
def test_not_served_falls_back(cuda, dtype, ci, co):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 5, 7, ci, generator=g).to(dtype).to(cuda)
    w = torch.randn(co, ci, 1, 1, generator=g).to(dtype).to(cuda)
    w2, y = w.reshape(co, ci).contiguous(), torch.empty(2, 5, 7, co, dtype=dtype, device=cuda)
    assert N.lib().mxr_pwconv_fwd(N._p(x), N._p(w2), N._p(y), 70, ci, co, N._dw_dt(x), N._s()) == -1
    with pytest.raises(N.NotServed):
        P.pointwise_conv(x, w, backend="native")
    assert not P.takes_native(x, co)
    if dtype != torch.float32:
        return      # torch ops on a bf16 12-channel channels-last view have segfaulted inside torch (README)
    with pytest.warns(UserWarning, match="pwconv.hip does not serve"):
        y = P.pointwise_conv(x, w)
    assert torch.equal(y, P.pointwise_conv_torch(x, w))


def test_captured_forward_backward_replays_bit_equal(cuda):
    g = torch.Generator().manual_seed(11)
    n, H, W, ci, co = 2, 17, 33, 24, 40
    w = torch.randn(co, ci, 1, 1, generator=g).to(cuda).requires_grad_()
    xs = [torch.randn(n, H, W, ci, generator=g).bfloat16().to(cuda) for _ in range(3)]
    x = xs[0].clone().requires_grad_()

    def step():
        y = N.PointwiseConvFn.apply(x, w)
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
    """C3..C5 and two pointwise weight gradients of MobileNet(0.25), bf16, 2 x 64 x 96: the native path may deviate
    from the float64 CPU run twice as far as the torch bf16 path does (27 batch-norms on tiny tensors: no bound can be
    derived; both round at the same points and the factor covers another accumulation order).  The torch bf16 path
    itself is 0.7 to 1.1 of max |ref| away on C5 and the two weight gradients, so only C3 and C4 constrain the native
    path here; the kernel cases above and the ``pw_taken`` assertion carry the checking."""
    torch.manual_seed(5)
    ref = MobileNet(0.25).double()
    ref.pw_backend = "torch"
    x = torch.randn(2, 64, 96, 3).bfloat16()

    def run(model, inp):
        outs = model(inp)
        sum(o.float().square().mean() for o in outs).backward()
        return [o.detach().double().cpu() for o in outs] + [model.pw[i].weight.grad.double().cpu() for i in (0, 12)]

    want = run(ref, x.double())
    dev = {}
    for backend in ("torch", "native"):
        m = MobileNet(0.25)
        m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        m.pw_backend = backend
        got = run(m.to(cuda), x.to(cuda))
        assert m.pw_taken == [backend] * 13
        dev[backend] = [float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, want)]
    names = ("C3", "C4", "C5", "dw conv_pw_1", "dw conv_pw_13")
    for name, t, nat in zip(names, dev["torch"], dev["native"]):
        print("\nMobileNet(0.25) {}: max |dev| / max |ref|: torch bf16 {:.3e}, native {:.3e}".format(name, t, nat))
    for name, t, nat in zip(names, dev["torch"], dev["native"]):
        assert nat <= 2.0 * t, name
