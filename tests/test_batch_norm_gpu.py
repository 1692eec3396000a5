"""``batch_norm.hip`` (``mxr_bn_stats / _act_fwd / _act_bwd``) against ``batch_norm_act_torch`` in float64 on the CPU.

Inputs are bf16-exact (x, dy) or fp32.  Tolerances and kink protocol are those of test_group_norm_gpu.py: bf16 outputs
get 2^-8 |ref| plus the fp32 term, fp32 outputs the fp32 term alone -- FP32_MARGIN = 8 times what PyTorch's fp32 CPU
batch norm + activation on a contiguous NCHW copy deviates from float64, per output, relative to its largest
magnitude.  Elements whose float64 pre-activation lies within KINK of 0 or 6 are left out of y / dx; asserted on the
oracle alone: they are at most 5e-4 of a case, none sits in a channel of 64 or fewer rows, and no pre-activation lies
within the flip bound of a kink.  ``offset60``: every channel 60 standard deviations from zero.
Mask agreement: bf16 rounds a pre-activation in [6 - 2^-6, 6), which still passes its gradient, to 6.0; dy is set
where y == 0, and where y == 6 and the oracle's pre-activation is above 6.  The fallback under one warning is run for
fp32 x only: for bf16 C = 12 the torch expression itself segfaulted inside torch on the GPU, cause not found, so that
case stops at the refusals.  The model factor 2 is taken from test_dwconv_gpu.py, not derived (27 norms, tiny tensors).
"""
import functools

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops import norm as norm_ops
from test_dwconv_gpu import SENTINEL, guarded
from test_group_norm_gpu import BF16_TERM, FLIP, FP32_MARGIN, KINK, KINK_SHARE, NEAR

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.01
SMALL, MID, BIG = (1, 1, 2), (3, 5, 7), (2, 37, 41)
# (C, NHW, act, variant): seed
CASES = {(C, s, "relu6", "plain"): 0 for C in (8, 24, 136, 1024) for s in (SMALL, MID, BIG) if C < 1024 or s != MID}
CASES.update({(24, MID, "none", "plain"): 0, (24, MID, "relu", "plain"): 0, (24, BIG, "relu6", "offset60"): 0})
KINKS = {"none": (), "relu": (0.0,), "relu6": (0.0, 6.0)}
OUTS = ("y", "mean", "rstd", "rmean", "rvar", "dx", "dgamma", "dbeta")


def torch_run(inp, training, act, dtype):
    """The torch expression with autograd in ``dtype`` on the CPU (float32: on a contiguous NCHW copy)."""
    x, dy, gamma, beta, rmean, rvar = (t.to(dtype).clone() for t in inp)
    [t.requires_grad_() for t in (x, gamma, beta)]
    xin = x if dtype == torch.float64 else x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    mean, rstd = rmean.clone(), 1.0 / torch.sqrt(rvar + EPS)
    if training:                                 # what the batch norm itself saves
        _, mean, rstd = torch.native_batch_norm(xin.detach().permute(0, 3, 1, 2), None, None, None, None, True, MOM, EPS)
    y = norm_ops.batch_norm_act_torch(xin, (gamma, beta, rmean, rvar), training, act, MOM, EPS)
    y.backward(dy)
    pre = (x.detach() - mean) * rstd * gamma.detach() + beta.detach()
    return dict(y=y.detach(), mean=mean, rstd=rstd, rmean=rmean, rvar=rvar, dx=x.grad, dgamma=gamma.grad,
                dbeta=beta.grad, pre=pre)


@functools.lru_cache(maxsize=None)
def reference(case, training):
    (C, nhw, act, variant), seed = case, CASES[case]
    g = torch.Generator().manual_seed(1000 * seed + C + nhw[1])
    x = torch.randn(*nhw, C, generator=g)
    rmean = 0.2 * torch.randn(C, generator=g)
    if variant == "offset60":
        off = 60.0 * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        x, rmean = x + off, rmean + off
    inp = (x.bfloat16().float(), torch.randn(*nhw, C, generator=g).bfloat16().float(), 2 + 0.25 * torch.randn(C, generator=g),
           3 + 0.5 * torch.randn(C, generator=g), rmean, 0.8 + 0.4 * torch.rand(C, generator=g))
    ref, f32 = torch_run(inp, training, act, torch.float64), torch_run(inp, training, act, torch.float32)
    dev = {k: float((f32[k].double() - r).abs().max() / r.abs().max().clamp_min(1e-300)) for k, r in ref.items()}
    dist = torch.stack([(ref["pre"] - k).abs() for k in KINKS[act]] + [torch.full_like(ref["pre"], 1e30)]).min(0).values
    near = dist < NEAR
    cond = dict(kink=dist < KINK, min_dist=float(dist.min()), mean_over_std=float((ref["mean"].abs() * ref["rstd"]).min()),
                pre_err=float((f32["pre"].double() - ref["pre"]).abs()[near].max()) if bool(near.any()) else 0.0)
    return dict(inp=inp, ref=ref, dev=dev, cond=cond)


def raw_run(case, training, dev):
    """The three entry points through ctypes, every output sentinel-filled and sentinel-followed."""
    C, nhw, act, _ = case
    x, dy, gamma, beta, rmean, rvar = (t.to(dev) for t in reference(case, training)["inp"])
    x, dy, n = x.bfloat16(), dy.bfloat16(), x.numel() // C
    nwork = N.lib().mxr_bn_work(n, C)
    b = {k: guarded(x.shape if k in ("y", "dx") else (nwork,) if k == "work" else (C,),
                    torch.bfloat16 if k in ("y", "dx") else torch.float32, dev) for k in OUTS + ("work",)}
    b["rmean"][0].copy_(rmean), b["rvar"][0].copy_(rvar)
    p = {k: N._p(v[0]) for k, v in b.items()}
    a = N.BN_ACTS[act]
    assert N.lib().mxr_bn_stats(N._p(x), p["rmean"], p["rvar"], p["mean"], p["rstd"], p["work"], nwork, n, C, EPS, MOM,
                                int(training), 1, N._s()) == 0
    assert N.lib().mxr_bn_act_fwd(N._p(x), N._p(gamma), N._p(beta), p["mean"], p["rstd"], p["y"], n, C, a, 1, N._s()) == 0
    assert N.lib().mxr_bn_act_bwd(N._p(dy), N._p(x), N._p(gamma), N._p(beta), p["mean"], p["rstd"], p["dx"], p["dgamma"],
                                  p["dbeta"], p["work"], nwork, n, C, a, int(training), 1, N._s()) == 0
    torch.cuda.synchronize()
    for k, (out, buf) in b.items():
        assert bool((buf[out.numel():] == SENTINEL).all()), "the row after {} was written".format(k)
    return {k: b[k][0] for k in OUTS}


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "C{}-{}x{}x{}-{}-{}".format(c[0], *c[1], *c[2:]))
def test_against_float64(cuda, case, training):
    C, nhw, act, variant = case
    n, rows = nhw[0] * nhw[1] * nhw[2], N.lib().mxr_bn_chunk_rows(C)
    r = reference(case, training)
    ref, dev, c = r["ref"], r["dev"], r["cond"]
    share = float(c["kink"].double().mean())
    print("\n{} training {}: {} rows in chunks of {}, kink share {:.1e}, nearest pre {:.2e}, fp32 pre error {:.2e}".format(
        case, training, n, rows, share, c["min_dist"], c["pre_err"]))
    assert share <= KINK_SHARE and c["min_dist"] >= max(FLIP, 2 * c["pre_err"]) and (n > 64 or not c["kink"].any())
    assert nhw != BIG or (n > rows and n % rows), "the largest shape must span chunks and end in a partial one"
    assert variant != "offset60" or c["mean_over_std"] > 50.0
    got = raw_run(case, training, cuda)
    for k, v in raw_run(case, training, cuda).items():
        assert torch.equal(v, got[k]), "repeat calls differ in " + k
    failed = []
    for k in OUTS:
        want = ref[k]
        allow = FP32_MARGIN * dev[k] * want.abs().max() + (BF16_TERM * want.abs() if k in ("y", "dx") else 0.0)
        err = (got[k].double().cpu() - want).abs()
        if k in ("y", "dx"):
            err = err.masked_fill(c["kink"], 0.0)
        ratio = float((err / (allow + 1e-300)).max())
        print("  {:6s} torch fp32 deviates {:.3e}; worst |err| / allowance {:.3f}".format(k, dev[k], ratio))
        if not bool((err <= allow).all()):
            failed.append(k)
    assert not failed, failed


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("C", (24, 136))
def test_mask_agreement(cuda, C, training):
    case = (C, BIG, "relu6", "plain")
    r = reference(case, training)
    assert r["cond"]["min_dist"] >= max(FLIP, 2 * r["cond"]["pre_err"])
    x, _, gamma, beta, rmean, rvar = (t.to(cuda) for t in r["inp"])
    x = x.bfloat16()
    mean, rstd = N.bn_stats(x, rmean, rvar, training, MOM, EPS)
    y = N.bn_act_fwd(x, gamma, beta, mean, rstd)
    clamped = (y == 0) | ((y == 6) & (r["ref"]["pre"] > 6).to(cuda))
    assert bool((y == 0).any()) and bool(((y == 6) & clamped).any()) and not bool(clamped.all())
    dx, dgamma, dbeta = N.bn_act_bwd(torch.where(clamped, 3.0, 0.0).bfloat16(), x, gamma, beta, mean, rstd, training)
    assert not dx.any() and not dgamma.any() and not dbeta.any()
    dx, dgamma, _ = N.bn_act_bwd(torch.where(clamped, 0.0, 3.0).bfloat16(), x, gamma, beta, mean, rstd, training)
    assert dx.any() and dgamma.any()                # and the complement passes


@pytest.mark.parametrize("dtype,C", ((torch.float32, 8), (torch.bfloat16, 12)))
def test_not_served(cuda, dtype, C):
    x = torch.randn(2, 5, 7, C, generator=torch.Generator().manual_seed(7)).to(dtype).to(cuda)
    bn = [t.to(cuda) for t in (torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C))]
    f = torch.full((4096,), SENTINEL, device=cuda)
    p, dt = N._p(f), N._dw_dt(x)
    assert N.lib().mxr_bn_stats(N._p(x), p, p, p, p, p, 4096, 70, C, EPS, MOM, 1, dt, N._s()) == -1
    assert N.lib().mxr_bn_act_fwd(N._p(x), p, p, p, p, p, 70, C, 2, dt, N._s()) == -1
    assert N.lib().mxr_bn_act_bwd(N._p(x), N._p(x), p, p, p, p, p, p, p, p, 4096, 70, C, 2, 1, dt, N._s()) == -1
    torch.cuda.synchronize()
    assert bool((f == SENTINEL).all())
    assert not norm_ops.bn_takes_native(x, True)
    with pytest.raises(N.NotServed):
        norm_ops.batch_norm_act(x, bn, True, backend="native", eps=EPS)
    assert bool((bn[2] == 0).all()) and bool((bn[3] == 1).all())
    if dtype != torch.float32:                   # see the module docstring
        return
    norm_ops._FALLBACK_WARNED.clear()
    want = norm_ops.batch_norm_act_torch(x, [t.clone() for t in bn], True, eps=EPS)
    with pytest.warns(UserWarning, match="batch_norm.hip does not serve C = 8") as rec:
        got = [norm_ops.batch_norm_act(x, bn, True, eps=EPS) for _ in range(2)]
    assert sum("batch_norm.hip" in str(w.message) for w in rec) == 1, "one warning per form"
    assert torch.equal(got[0], want) and not bool((bn[2] == 0).all())


def test_captured_forward_backward_replays_bit_equal(cuda):
    g, C = torch.Generator().manual_seed(11), 24
    ga, be = ((o + 0.25 * torch.randn(C, generator=g)).to(cuda).requires_grad_() for o in (2, 3))
    stats = [torch.zeros(C, device=cuda), torch.ones(C, device=cuda)]
    xs = [torch.randn(*BIG, C, generator=g).bfloat16().to(cuda) for _ in range(3)]
    x = xs[0].clone().requires_grad_()

    def step(rmean, rvar):
        y = norm_ops.batch_norm_act(x, (ga, be, rmean, rvar), True, "relu6", "native", MOM, EPS)
        return (y,) + torch.autograd.grad(y, (x, ga, be), torch.ones_like(y) * 0.5)

    step(*stats)                                 # warm-up outside the capture, on the current stream
    eager = [t.clone() for t in stats]           # capturing launches nothing: both chains start here
    graph = torch.cuda.CUDAGraph()
    # as train/step_graphs.py captures: thread-local mode, the shared capture stream, no stream of the test's own
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = step(*stats)
    for new in xs[1:] + xs[1:]:                  # several replays on new input; the running statistics accumulate
        with torch.no_grad():
            x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        for a, b in zip(got + stats, list(step(*eager)) + eager):
            assert torch.equal(a, b)
    assert not torch.equal(stats[0], torch.zeros_like(stats[0]))
    torch.cuda.synchronize()                     # no replay in flight when the graph and its pool go


def test_mobilenet_native_against_float64(cuda):
    torch.manual_seed(5)
    ref = MobileNet(0.25).double()
    ref.dw_backend = ref.bn_backend = "torch"
    x = torch.randn(2, 64, 96, 3).bfloat16()
    bns = lambda m: [m.conv1_bn] + [b for pair in zip(m.dw_bn, m.pw_bn) for b in pair]      # noqa: E731

    def run(model, inp):
        outs = model(inp)
        sum(o.float().square().mean() for o in outs).backward()
        return [t.detach().double().cpu() for t in outs + [model.dw_bn[0].bn.weight.grad] + [b.bn.running_mean for b in bns(model)]]

    want = run(ref, x.double())
    dev = {}
    for backend in ("torch", "native"):
        m = MobileNet(0.25)
        m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()}, strict=True)
        for b in bns(m):                         # ref has stepped once: start from fresh statistics, as it did
            b.bn.reset_running_stats()
        m.bn_backend = backend
        got = run(m.to(cuda), x.to(cuda))
        assert m.bn_taken == [backend] * 27 and all(int(b.bn.num_batches_tracked) == 1 for b in bns(m))
        dev[backend] = [float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, want)]
    names = ["C3", "C4", "C5", "dgamma conv_dw_1_bn"] + ["running mean {}".format(i) for i in range(27)]
    for name, t, nat in zip(names, dev["torch"], dev["native"]):
        print("\nMobileNet(0.25) {}: max |dev| / max |ref|: torch bf16 {:.3e}, native {:.3e}".format(name, t, nat))
    assert not [name for name, t, nat in zip(names, dev["torch"], dev["native"]) if nat > 2.0 * t]
