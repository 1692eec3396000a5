"""The fused Keras-Adam kernel with its bf16 compute copies, ``mxr_refresh_copy``, the gradient norm / clip
factor and ``mxr_scale_inplace`` (csrc/kernels/optim.hip) against float64 Keras Adam (the
header of optim.hip), over segments that cross chunks (AdamPlan.CHUNK = 8192), leave scalar tails and have
4-vectors straddling two output channels.  The compute copies are checked bit for bit."""
import math

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.train.flat import FlatParams
from batchai_retinanet_horovod_coco_amd.train.optimizer import KerasAdam

pytestmark = pytest.mark.gpu

# shape, has a per-output-channel scale
PARAMS = [
    ((7, 3, 3, 5), True),      # row length 45: 4-vectors straddle rows
    ((13,), False),            # three vectors and a scalar tail, no scale
    ((64, 1, 1, 64), True),
    ((3, 8195), True),         # 24,585 = 3 x 8192 + 9: a last chunk of two vectors and a scalar tail; the row
                               # boundaries fall inside chunks and inside vectors
    ((2, 8192), False),        # exactly two whole chunks
]
SENTINEL = -12345.0
B1, B2, EPS = (float(np.float32(v)) for v in (0.9, 0.999, 1e-7))     # as the kernel receives them (fp32)


class _BN:
    def __init__(self, scale):
        self.scale = scale

    def scale_shift(self):
        return self.scale, None


class _Conv:
    """What ComputeWeights.build reads of a conv layer: its weight and its frozen-BN scale."""

    def __init__(self, weight, scale):
        self.weight = weight
        self.bn = None if scale is None else _BN(scale)


class Setup:
    def __init__(self, dev, seed, lr, clipnorm):
        gen = torch.Generator().manual_seed(seed)
        self.gen = gen
        self.params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s, _ in PARAMS]
        self.scales = [(torch.rand(s[0], generator=gen) + 0.5).to(dev) if sc else None for s, sc in PARAMS]
        self.flat = FlatParams([(str(i), p) for i, p in enumerate(self.params)])
        # registers its AdamPlan (copy=True, scales) for this flat buffer: KerasAdam.step() below uses it
        self.cw = N.ComputeWeights(self.flat, [_Conv(p, s) for p, s in zip(self.params, self.scales)])
        self.plan = self.cw.plan
        assert N.adam_plan(self.flat) is self.plan and self.plan.copy is not None
        assert self.plan.nchunks == 1 + 1 + 1 + 4 + 2
        self.opt = KerasAdam(self.flat, lr=lr, clipnorm=clipnorm)
        self.pad = torch.ones(self.flat.total, dtype=torch.bool, device=dev)
        for s in self.flat.segments:
            self.pad[s.offset:s.offset + s.numel] = False
        assert int(self.pad.sum()) == 5 + 51 + 55
        for buf in (self.flat.data, self.opt.m, self.opt.v):
            buf[self.pad] = SENTINEL
        self.plan.copy[self.pad] = SENTINEL
        # float64 state
        self.p64 = self.flat.data.double().cpu()
        self.m64 = torch.zeros_like(self.p64)
        self.v64 = torch.zeros_like(self.p64)
        self.t = 0

    def close(self):
        N._PLANS.pop(id(self.flat), None)

    def new_grad(self):
        g = torch.randn(self.flat.total, generator=self.gen)
        g[self.pad.cpu()] = 0          # the padding carries no gradient
        self.flat.grad.copy_(g)
        return g.double()

    def ref_step(self, g, lr, clipnorm):
        """One float64 Keras-Adam step; returns the pre-clip global norm."""
        norm = math.sqrt(float((g * g).sum()))
        if clipnorm and clipnorm > 0 and norm >= clipnorm:
            g = g * (float(np.float32(clipnorm)) / norm)
        self.t += 1
        lr_t = float(np.float32(lr)) * math.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t)
        self.m64 = B1 * self.m64 + (1.0 - B1) * g
        self.v64 = B2 * self.v64 + (1.0 - B2) * g * g
        self.p64 = self.p64 - lr_t * self.m64 / (self.v64.sqrt() + EPS)
        return norm

    def check_state(self):
        for s in self.flat.segments:
            a = slice(s.offset, s.offset + s.numel)
            assert torch.allclose(self.flat.data[a].cpu().double(), self.p64[a], atol=1e-6, rtol=1e-5), s.shape
            assert torch.allclose(self.opt.m[a].cpu().double(), self.m64[a], atol=1e-7, rtol=1e-5), s.shape
            assert torch.allclose(self.opt.v[a].cpu().double(), self.v64[a], atol=1e-7, rtol=1e-5), s.shape

    def check_copy(self):
        """Every compute copy is exactly bf16(p * scale of its output channel): one fp32 multiply and one
        round-to-nearest-even, so any difference is an indexing error."""
        for s, sc in zip(self.flat.segments, self.scales):
            p = self.flat.data[s.offset:s.offset + s.numel].view(s.shape[0], -1)
            want = (p * sc[:, None] if sc is not None else p).bfloat16().reshape(-1)
            got = self.plan.copy[s.offset:s.offset + s.numel]
            bad = (got != want).nonzero().flatten()
            assert bad.numel() == 0, "compute copy of segment {} (row length {}): {} elements differ, first at {}".format(
                s.shape, s.numel // s.shape[0], bad.numel(), bad[:8].tolist())
            assert self.cw.get(s.param).data_ptr() == got.data_ptr()

    def check_padding(self):
        for name, buf in (("data", self.flat.data), ("m", self.opt.m), ("v", self.opt.v), ("copy", self.plan.copy)):
            assert bool((buf[self.pad].float() == torch.tensor(SENTINEL).to(buf.dtype).float().item()).all()), name


@pytest.fixture
def make_setup(cuda):
    made = []

    def make(seed, lr=1e-3, clipnorm=0.5):
        made.append(Setup(cuda, seed, lr, clipnorm))
        return made[-1]

    yield make
    for s in made:
        s.close()


# the gradient norm is about sqrt(45,393) = 213
@pytest.mark.parametrize("clipnorm,lrs", [
    (0.5, [1e-3] * 5),                          # clip active
    (1e6, [1e-3] * 5),                          # far above the norm: factor exactly 1
    (0.0, [1e-3] * 5),                          # no clipping
    (0.5, [1e-3, 1e-3, 2.5e-4, 2.5e-4, 2.5e-4]),  # the learning rate changes between steps 2 and 3
], ids=["clip", "clip_inactive", "clip_off", "lr_change"])
def test_adam_steps(make_setup, clipnorm, lrs):
    st = make_setup(seed=41, lr=lrs[0], clipnorm=clipnorm)
    st.check_copy()                             # as built (ComputeWeights.build -> mxr_refresh_copy)
    for lr in lrs:
        g = st.new_grad()
        st.opt.lr = lr
        if clipnorm != 0.5:
            _, factor = st.opt.norm_and_scale()
            assert factor.item() == 1.0
        norm = st.opt.step()
        ref_norm = st.ref_step(g, lr, clipnorm)
        assert abs(norm.item() - ref_norm) <= 1e-5 * ref_norm
        assert (ref_norm >= clipnorm > 0) == (clipnorm == 0.5)
        st.check_state()
        st.check_copy()
    assert st.opt.iterations == 5 and st.plan.iter.item() == 5
    st.check_padding()


def test_refresh_copy(make_setup):
    """mxr_refresh_copy after the weights were replaced (checkpoint load, broadcast)."""
    st = make_setup(seed=42)
    new = torch.randn(st.flat.total, generator=st.gen).to(st.flat.data.device)
    st.flat.data.copy_(torch.where(st.pad, st.flat.data, new))
    st.plan.copy[~st.pad] = 0
    gen0 = st.plan.generation
    st.cw.refresh()
    assert st.plan.generation == gen0 + 1
    st.check_copy()
    st.check_padding()


def test_grad_norm_clip_and_scale(cuda):
    """3 x 2^20 + 3 elements > 1024 x 256 x 4: the grid-stride trip and the scalar tail of sumsq_kernel and
    scale_kernel."""
    n = 3 * 2 ** 20 + 3
    g = torch.randn(n, generator=torch.Generator().manual_seed(43)).to(cuda)
    g[-3:] = torch.tensor([30.0, -40.0, 50.0], device=cuda)        # the tail weighs in: 5,000 of ~3.15 M
    ref = math.sqrt(float((g.double() ** 2).sum().item()))
    for clipnorm, norm_mul, scale_mul in [(0.0, 1.0, 1.0), (7.0, 1.0, 0.25), (1e9, 1.0, 0.5), (7.0, 0.5, 1.0)]:
        out = N.grad_norm_clip(g, norm_mul, clipnorm, scale_mul)
        norm = ref * norm_mul
        factor = (clipnorm / norm if clipnorm > 0 and norm >= clipnorm else 1.0) * scale_mul
        assert abs(out[0].item() - norm) <= 1e-5 * norm
        assert abs(out[1].item() - factor) <= 1e-5 * factor
        if not (clipnorm > 0 and norm >= clipnorm):
            assert out[1].item() == scale_mul
    assert abs(N.l2norm(g).item() - ref) <= 1e-5 * ref
    s = torch.tensor([0.3717], device=cuda)
    want = g * s
    N.scale_inplace(g, s)
    assert torch.equal(g, want)
