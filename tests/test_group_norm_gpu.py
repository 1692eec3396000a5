"""``group_norm.hip`` (``mxr_gn_relu_fwd`` / ``mxr_gn_relu_bwd``) against the float64 torch expression.

Every case runs on the ragged levels S = [(37,41), (5,7), (3,4), (2,2), (1,1)]: the first level is cut into twelve
128-pixel chunks (several blocks per segment, a partial last chunk, several row trips per thread), the last one is a
single pixel with 8 or 16 elements per group.  Inputs are bf16-exact (x, dy) or fp32 (gamma, beta), so the float64
oracle reads exactly what the kernels read.

Tolerances.  The bf16 outputs y and dx may differ from float64 by 2^-8 * |value| (twice bf16's half-ulp: rounding an
fp32 result that is itself off) plus the fp32 term; the fp32 outputs by the fp32 term alone.  The fp32 term is
measured, not fixed: what PyTorch's own fp32 group norm + ReLU on the CPU deviates from float64 on the same inputs,
per output, relative to that output's largest magnitude -- the kernel is allowed FP32_MARGIN = 8 times that (the
margin test_iou_loss_gpu.py sets for a kernel against fp32 autograd).

The kink.  Elements whose float64 pre-activation lies within KINK = 1e-4 of zero are left out of the y / dx
comparison (their mask is legitimately undecided).  Asserted on the oracle alone: they are at most 5e-4 of all
elements, none lies in a segment with 64 or fewer elements per group (there one flipped mask moves the whole group's
dx), and no pre-activation at all lies within the case's flip bound of zero: twice what the CPU's fp32 pre-activation
deviates from the float64 one around the kink (measured per case), and at least FLIP = 2e-6.  The fp32 pre-activation
is a handful of roundings away from the float64 one, so outside that bound the kernel's mask is the oracle's and no
group's sums s1 / s2 lose or gain a term.  The seeds below were chosen on the CPU to meet all three.

The cancellation case, offset60, puts every channel of a group 60 standard deviations from zero (the sign drawn per
group), so |mean| * rstd is about 60 in every (image, level, group) -- asserted -- and a variance taken as
E[x^2] - mean^2 in fp32 loses three to four digits.  The fp32 yardstick moves with it: 7e-7 to 6e-6 for y, dx and
dgamma against 2e-7 to 4e-7 in the other cases, and a kink share of 2.4e-4 against 1e-4.  It runs at (C, G) = (64, 8)
because its flip bound is about 5e-6 and no seed keeps the 1.2 million pre-activations of a 256-channel case outside
that.

The model-level check compares the packed bf16 HIP heads with the same weights on the torch backend (bf16 list path,
``F.group_norm`` per level): the two losses within 2 % and the head gradients next to the loss at a cosine of 0.95 --
the bars test_model_parity_gpu.py sets for the bf16 HIP path against torch.
"""
import ctypes
import functools

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops import norm as norm_ops

pytestmark = pytest.mark.gpu

S = [(37, 41), (5, 7), (3, 4), (2, 2), (1, 1)]
NPIX = [h * w for h, w in S]
P = sum(NPIX)
EPS = 1e-5
KINK = 1e-4
KINK_SHARE = 5e-4
FLIP = 2e-6
NEAR = 1e-2             # where the fp32 error of the pre-activation is measured: around the kink
FP32_MARGIN = 8.0
BF16_TERM = 2.0 ** -8
SENTINEL = 12288.0      # exact in bf16

# name: (C, G, B, seed, variant)
CASES = {
    "c64_g8": (64, 8, 3, 0, "plain"),
    "c256_g32": (256, 32, 3, 3, "plain"),
    "c256_g16": (256, 16, 2, 0, "plain"),
    "offset60": (64, 8, 3, 0, "offset"),
    "gamma0": (64, 8, 3, 0, "gamma0"),
    "zero_level": (64, 8, 3, 0, "zero_level"),
}


def make_inputs(name):
    """(x bf16-exact f32, dy bf16-exact f32, gamma f32, beta f32) on the CPU."""
    C, G, B, seed, variant = CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(B, P, C, generator=g) * 1.5 + 0.3
    if variant == "offset":
        # every channel of a group sits 60 standard deviations from zero, the sign drawn per group: |mean| * rstd is
        # about 60 in every (image, level, group), the regime in which E[x^2] - mean^2 loses its digits
        sign = torch.where(torch.rand(G, generator=g) < 0.5, -1.0, 1.0).repeat_interleave(C // G)
        x = torch.randn(B, P, C, generator=g) + 60.0 * sign
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(B, P, C, generator=g)
    if variant == "gamma0":
        gamma[::3] = 0.0
    if variant == "zero_level":
        x[:, NPIX[0]:NPIX[0] + NPIX[1]] = 0.0
    return x.bfloat16().float(), dy.bfloat16().float(), gamma, beta


def _stats(x, G):
    """mean, rstd [B, L, G] and the pre-activation-free normalised input, in x's dtype."""
    B, _, C = x.shape
    means, rstds, off = [], [], 0
    for n in NPIX:
        v = x[:, off:off + n].reshape(B, n, G, C // G)
        m = v.mean(dim=(1, 3))
        var = ((v - m[:, None, :, None]) ** 2).mean(dim=(1, 3))
        means.append(m)
        rstds.append(1.0 / torch.sqrt(var + EPS))
        off += n
    return torch.stack(means, 1), torch.stack(rstds, 1)


def _pre(x, gamma, beta, mean, rstd, G):
    B, _, C = x.shape
    out, off = [], 0
    for l, n in enumerate(NPIX):
        v = x[:, off:off + n].reshape(B, n, G, C // G)
        xh = (v - mean[:, l][:, None, :, None]) * rstd[:, l][:, None, :, None]
        out.append(xh.reshape(B, n, C) * gamma + beta)
        off += n
    return torch.cat(out, 1)


def _torch_run(x, dy, gamma, beta, G, dtype):
    """The torch expression with autograd in ``dtype`` on the CPU: y, dx, dgamma, dbeta (and mean / rstd from
    native_group_norm per level, what F.group_norm itself computes)."""
    x = x.to(dtype).clone().requires_grad_(True)            # (clones: the cached inputs stay plain tensors)
    gamma = gamma.to(dtype).clone().requires_grad_(True)
    beta = beta.to(dtype).clone().requires_grad_(True)
    y = norm_ops.group_norm_relu_packed(x, S, gamma, beta, G, EPS)
    y.backward(dy.to(dtype))
    B, _, C = x.shape
    means, rstds, off = [], [], 0
    with torch.no_grad():
        for (h, w), n in zip(S, NPIX):
            lv = x[:, off:off + n].reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous()
            _, m, r = torch.native_group_norm(lv, gamma, beta, B, C, n, G, EPS)
            means.append(m.reshape(B, G))
            rstds.append(r.reshape(B, G))
            off += n
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, mean=torch.stack(means, 1),
                rstd=torch.stack(rstds, 1))


def oracle_conditions(name):
    """The oracle-only figures of a case (used to choose the seeds, asserted by the tests)."""
    C, G, B, _, _ = CASES[name]
    x, dy, gamma, beta = make_inputs(name)
    m64, r64 = _stats(x.double(), G)
    pre64 = _pre(x.double(), gamma.double(), beta.double(), m64, r64, G)
    m32, r32 = _stats(x, G)
    pre32 = _pre(x, gamma, beta, m32, r32, G)
    kink = pre64.abs() < KINK
    small, off = torch.zeros(P, dtype=torch.bool), 0
    for n in NPIX:
        if n * (C // G) <= 64:
            small[off:off + n] = True
        off += n
    return dict(kink=kink, share=kink.double().mean().item(), in_small=int(kink[:, small].sum()),
                min_pre=pre64.abs().min().item(),
                mean_over_std=((m64.abs() * r64).min().item(), (m64.abs() * r64).max().item()),
                fp32_pre_err=(pre32.double() - pre64).abs()[pre64.abs() < NEAR].max().item(), pre64=pre64)


@functools.lru_cache(maxsize=None)
def reference(name):
    C, G, B, _, _ = CASES[name]
    x, dy, gamma, beta = make_inputs(name)
    ref = _torch_run(x, dy, gamma, beta, G, torch.float64)
    m64, r64 = _stats(x.double(), G)
    assert torch.allclose(ref["mean"], m64, rtol=1e-12, atol=1e-12) and torch.allclose(ref["rstd"], r64, rtol=1e-12)
    f32 = _torch_run(x, dy, gamma, beta, G, torch.float32)
    dev = {}
    for k, r in ref.items():
        dev[k] = ((f32[k].double() - r).abs().max() / r.abs().max().clamp_min(1e-300)).item()
    cond = oracle_conditions(name)
    return dict(inputs=(x, dy, gamma, beta), ref=ref, dev=dev, cond=cond)


def _lev():
    flat, off = [], 0
    for n in NPIX:
        flat += [off, n]
        off += n
    return (ctypes.c_int * len(flat))(*flat)


def _guarded(numel, dtype, dev):
    """A buffer of ``numel`` elements with 64 sentinel elements behind it."""
    buf = torch.full((numel + 64,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[:numel]


def _blocks(B):
    rows = N.lib().mxr_gn_chunk_rows()
    return B * sum((n + rows - 1) // rows for n in NPIX)


def raw_run(cuda, name):
    """Both entry points on buffers with sentinels behind every output and workspace."""
    C, G, B, _, _ = CASES[name]
    x, dy, gamma, beta = (t.to(cuda) for t in reference(name)["inputs"])
    xb, dyb = x.bfloat16().contiguous(), dy.bfloat16().contiguous()
    L = len(NPIX)
    bufs = {}
    for k, (n, dt) in dict(y=(B * P * C, torch.bfloat16), dx=(B * P * C, torch.bfloat16), mean=(B * L * G, torch.float32),
                           rstd=(B * L * G, torch.float32), dgamma=(C, torch.float32), dbeta=(C, torch.float32),
                           part=(2 * _blocks(B) * G, torch.float32),
                           work=(2 * _blocks(B) * (G + C) + 2 * B * L * G, torch.float32)).items():
        bufs[k] = _guarded(n, dt, cuda)
    p = lambda k: bufs[k][1].data_ptr()      # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    rc = N.lib().mxr_gn_relu_fwd(xb.data_ptr(), gamma.data_ptr(), beta.data_ptr(), p("y"), p("mean"), p("rstd"),
                                 p("part"), bufs["part"][1].numel(), B, P, C, G, EPS, L, _lev(), 1, s)
    assert rc == 0
    rc = N.lib().mxr_gn_relu_bwd(dyb.data_ptr(), xb.data_ptr(), gamma.data_ptr(), beta.data_ptr(), p("mean"), p("rstd"),
                                 p("dx"), p("dgamma"), p("dbeta"), p("work"), bufs["work"][1].numel(), B, P, C, G, L,
                                 _lev(), 1, s)
    assert rc == 0
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert bool((buf[view.numel():].float() == SENTINEL).all()), "sentinel behind {} overwritten".format(k)
    out = {k: bufs[k][1].clone() for k in ("y", "dx", "mean", "rstd", "dgamma", "dbeta")}
    out["y"] = out["y"].reshape(B, P, C)
    out["dx"] = out["dx"].reshape(B, P, C)
    out["mean"] = out["mean"].reshape(B, L, G)
    out["rstd"] = out["rstd"].reshape(B, L, G)
    return out, (xb, dyb, gamma, beta)


def _check_oracle_conditions(name):
    C, G, B, _, _ = CASES[name]
    c = reference(name)["cond"]
    print("{}: kink share {:.2e} ({} in small segments), min |pre| {:.2e}, fp32 pre error on the CPU {:.2e}".format(
        name, c["share"], c["in_small"], c["min_pre"], c["fp32_pre_err"]))
    assert c["share"] <= KINK_SHARE
    assert c["in_small"] == 0
    assert c["min_pre"] >= max(FLIP, 2 * c["fp32_pre_err"])
    if CASES[name][4] == "offset":
        print("{}: |mean| * rstd between {:.1f} and {:.1f}".format(name, *c["mean_over_std"]))
        assert c["mean_over_std"][0] >= 40.0
    return c["kink"]


@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(cuda, name):
    C, G, B, _, variant = CASES[name]
    r = reference(name)
    kink = _check_oracle_conditions(name)
    got, _ = raw_run(cuda, name)
    ref, dev = r["ref"], r["dev"]
    assert all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    if variant == "zero_level":
        assert torch.equal(got["mean"][:, 1].cpu(), torch.zeros(B, G))
        assert torch.allclose(got["rstd"][:, 1].cpu(), torch.full((B, G), EPS ** -0.5), rtol=1e-6)
    lines, failed = [], []
    for k in ("mean", "rstd", "y", "dx", "dgamma", "dbeta"):
        g64, want = got[k].double().cpu(), ref[k]
        allow = FP32_MARGIN * dev[k] * want.abs().max()
        tol = allow + (BF16_TERM * want.abs() if k in ("y", "dx") else 0.0)
        err = (g64 - want).abs()
        if k in ("y", "dx"):
            err = err.masked_fill(kink, 0.0)
        excess = (err - tol).max().item()
        worst = (err / want.abs().max()).max().item()
        lines.append("{:11s} {:6s} torch fp32 deviates {:.3e}, allowance {:.3e}, kernel worst |err| / max {:.3e}{}".format(
            name, k, dev[k], FP32_MARGIN * dev[k], worst, "" if excess <= 0 else "  EXCEEDS by {:.3e}".format(excess)))
        if excess > 0:
            failed.append(k)
    print("\n" + "\n".join(lines))
    assert not failed, failed


@pytest.mark.parametrize("name", ["c64_g8", "c256_g16"])
def test_two_calls_and_the_wrapper_give_the_same_bits(cuda, name):
    C, G, B, _, _ = CASES[name]
    a, (xb, dyb, gamma, beta) = raw_run(cuda, name)
    b, _ = raw_run(cuda, name)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    x = xb.clone().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = norm_ops.group_norm_relu(x, S, ga, be, G, EPS)
    assert isinstance(y.grad_fn, N.GroupNormReluPackedFn._backward_cls)
    y.backward(dyb)
    torch.cuda.synchronize()
    assert ga.grad.dtype == torch.float32 and be.grad.dtype == torch.float32
    assert torch.equal(y.detach(), a["y"]) and torch.equal(x.grad, a["dx"])
    assert torch.equal(ga.grad, a["dgamma"]) and torch.equal(be.grad, a["dbeta"])


@pytest.mark.parametrize("name", ["c256_g32", "gamma0"])
def test_mask_agreement(cuda, name):
    """dy non-zero only where the forward wrote 0: the backward's recomputed mask must drop every element."""
    C, G, B, _, _ = CASES[name]
    x, _, gamma, beta = (t.to(cuda) for t in reference(name)["inputs"])
    xb = x.bfloat16()
    y, mean, rstd = N.gn_relu_fwd(xb, S, gamma, beta, G, EPS)
    assert 0.2 < (y == 0).float().mean().item() < 0.8
    dy = torch.where(y == 0, torch.full_like(y, 3.0), torch.zeros_like(y))
    dx, dgamma, dbeta = N.gn_relu_bwd(dy, xb, S, gamma, beta, mean, rstd, G)
    torch.cuda.synchronize()
    assert not dx.any() and not dgamma.any() and not dbeta.any()
    # and the complement passes: the same call with dy where the forward wrote something is not zero
    dx2, dgamma2, _ = N.gn_relu_bwd(torch.where(y != 0, torch.full_like(y, 3.0), torch.zeros_like(y)), xb, S, gamma, beta,
                                    mean, rstd, G)
    assert dx2.any() and dgamma2.any()


def test_refusals_fall_back_to_the_torch_expression(cuda):
    def entry(C, G, nlev=5, dtype=1, B=2):
        lev = (ctypes.c_int * (2 * max(nlev, 1)))(*sum(([i * 4, 4] for i in range(max(nlev, 1))), []))
        Pn = 4 * nlev
        x = torch.zeros(B * Pn * C + 64, dtype=torch.bfloat16, device=cuda)
        y = torch.full_like(x, SENTINEL)
        f = torch.full((4096,), SENTINEL, dtype=torch.float32, device=cuda)
        ga = torch.ones(C, device=cuda)
        rc = N.lib().mxr_gn_relu_fwd(x.data_ptr(), ga.data_ptr(), ga.data_ptr(), y.data_ptr(), f.data_ptr(),
                                     f[1024:].data_ptr(), f[2048:].data_ptr(), 2048, B, Pn, C, G, EPS, nlev, lev, dtype,
                                     torch.cuda.current_stream().cuda_stream)
        rb = N.lib().mxr_gn_relu_bwd(x.data_ptr(), x.data_ptr(), ga.data_ptr(), ga.data_ptr(), f.data_ptr(),
                                     f[1024:].data_ptr(), y.data_ptr(), f[2048:].data_ptr(), f[2048 + C:].data_ptr(),
                                     f[3072:].data_ptr(), 0, B, Pn, C, G, nlev, lev, dtype,
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        untouched = bool((y.float() == SENTINEL).all()) and bool((f == SENTINEL).all())
        return rc, rb, untouched

    assert entry(96, 4) == (-1, -1, True)           # 24 channels per group
    assert entry(64, 16) == (-1, -1, True)          # 4 channels per group
    assert entry(36, 3) == (-1, -1, True)           # C % 8 != 0
    assert entry(64, 8, nlev=6) == (-1, -1, True)   # more than 5 levels
    assert entry(64, 8, dtype=0) == (-1, -1, True)  # fp32 activations
    assert entry(64, 8, dtype=2) == (-1, -1, True)
    rc, rb, untouched = entry(64, 8)
    assert rc == 0 and rb == -2 and not untouched   # the served form runs (and a short workspace is refused)

    g = torch.Generator().manual_seed(5)
    for C, G, dt in ((96, 4, torch.bfloat16), (64, 8, torch.float32)):
        x = torch.randn(2, P, C, generator=g).to(cuda, dt).requires_grad_(True)
        ga = (1 + 0.5 * torch.randn(C, generator=g)).to(cuda).requires_grad_(True)
        be = (0.3 * torch.randn(C, generator=g)).to(cuda).requires_grad_(True)
        y = norm_ops.group_norm_relu(x, S, ga, be, G, EPS)
        assert not isinstance(y.grad_fn, N.GroupNormReluPackedFn._backward_cls)
        want = norm_ops.group_norm_relu_packed(x, S, ga, be, G, EPS)
        assert torch.equal(y, want) and y.dtype == dt
        y.float().sum().backward()
        assert x.grad is not None and ga.grad is not None and be.grad is not None


def test_model_heads_agree_with_the_torch_backend(cuda):
    """The whole model, bf16: packed HIP heads with the fused GroupNorm against the torch backend (list path,
    F.group_norm per level) on the same weights and batch."""
    from batchai_retinanet_horovod_coco_amd import models
    from batchai_retinanet_horovod_coco_amd.data.synthetic import make_batch
    from batchai_retinanet_horovod_coco_amd.ops import conv as conv_ops
    from batchai_retinanet_horovod_coco_amd.train.engine import Trainer

    torch.manual_seed(0)
    ref_model = models.backbone("resnet18").retinanet(8, head_norm="gn")
    with torch.no_grad():
        for n in ref_model.norms():
            n.gamma.add_(0.2 * torch.randn_like(n.gamma))
            n.beta.add_(0.2 * torch.randn_like(n.beta))
    state = {k: v.clone() for k, v in ref_model.state_dict().items()}
    batch = make_batch(2, 128, 192, num_classes=8, generator=torch.Generator().manual_seed(7))

    def run(hip):
        if hip:
            N.enable()
            conv_ops.set_conv_backend("auto")
        else:
            N.disable()
            conv_ops.set_conv_backend("torch")
        try:
            model = models.backbone("resnet18").retinanet(8, head_norm="gn")
            model.load_state_dict(state)
            tr = Trainer(model, compute_dtype=torch.bfloat16, clip_mode="global", device=cuda)
            tr.optimizer.zero_grad()
            b = {k: v.to(cuda) for k, v in batch.items()}
            reg, cls = tr.forward_backward(b["images"], b["gt"], b["gt_count"], b["image_hw"])
            torch.cuda.synchronize()
            grads = {s.name: tr.flat.grad[s.offset:s.offset + s.numel].double().clone() for s in tr.flat.segments}
            tr.optimizer.remove_hooks()
            return float(reg), float(cls), grads
        finally:
            N.set_grad_sinks(None)
            N.set_compute_weights(None)
            N.enable()
            conv_ops.set_conv_backend("auto")

    r_t, c_t, g_t = run(False)
    r_h, c_h, g_h = run(True)
    print("\nlosses torch bf16: reg {:.5f} cls {:.5f} | HIP bf16: reg {:.5f} cls {:.5f}".format(r_t, c_t, r_h, c_h))
    assert abs(r_h - r_t) <= 0.02 * abs(r_t) and abs(c_h - c_t) <= 0.02 * abs(c_t)
    # next to the loss, and at the bottom of the towers: those gradients have gone through every GroupNorm's dx and
    # the tower convs' unmasked data gradients
    names = [n for n in g_t if n.endswith("submodel.final.weight") or n.endswith("submodel.final.bias")
             or ".norms.3." in n or ".norms.0." in n or n.endswith("submodel.tower.0.weight")
             or n.endswith("submodel.tower.0.bias")]
    assert len(names) == 16
    for name in names:
        a, b = g_t[name], g_h[name]
        assert bool(b.any()), name
        c = float(torch.dot(a, b) / (a.norm() * b.norm()))
        print("{:45s} cosine {:.5f}".format(name, c))
        assert c >= 0.95, name
