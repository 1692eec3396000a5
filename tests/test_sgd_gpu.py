"""The fused Keras-SGD kernel (``mxr_sgd_step``, csrc/kernels/optim.hip) with its bf16 compute copies against a
float64 evaluation of the update rule -- momentum, nesterov, coupled weight decay on the rank >= 2 segments, and the
learning rate and the momentum read from device memory -- over the segments of tests/test_optim_gpu.py: rows that
straddle 4-vectors, segments that cross chunks (AdamPlan.CHUNK = 8192), scalar tails and exactly full chunks.  The
compute copies are checked bit for bit."""
import math

import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.train.flat import FlatParams
from batchai_retinanet_horovod_coco_amd.train.optimizer import KerasSGD

pytestmark = pytest.mark.gpu

# shape, has a per-output-channel scale
PARAMS = [
    ((7, 3, 3, 5), True),      # row length 45: 4-vectors straddle rows
    ((13,), False),            # three vectors and a scalar tail, no scale; rank 1: never decayed
    ((64, 1, 1, 64), True),
    ((3, 8195), True),         # 24,585 = 3 x 8192 + 9: a last chunk of two vectors and a scalar tail
    ((2, 8192), False),        # exactly two whole chunks
]
SENTINEL = -12345.0
STEPS = 5


def f32(x):
    return float(np.float32(x))


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
    def __init__(self, dev, seed, backend="auto", **opt):
        gen = torch.Generator().manual_seed(seed)
        self.gen = gen
        self.params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s, _ in PARAMS]
        self.scales = [(torch.rand(s[0], generator=gen) + 0.5).to(dev) if sc else None for s, sc in PARAMS]
        self.flat = FlatParams([(str(i), p) for i, p in enumerate(self.params)])
        # registers its AdamPlan (copy=True, scales) for this flat buffer: the SGD step below uses it
        self.cw = N.ComputeWeights(self.flat, [_Conv(p, s) for p, s in zip(self.params, self.scales)])
        self.plan = self.cw.plan
        assert N.adam_plan(self.flat) is self.plan and self.plan.copy is not None
        assert self.plan.nchunks == 1 + 1 + 1 + 4 + 2
        self.opt = KerasSGD(self.flat, backend=backend, **opt)
        self.pad = torch.ones(self.flat.total, dtype=torch.bool, device=dev)
        for s in self.flat.segments:
            self.pad[s.offset:s.offset + s.numel] = False
        assert int(self.pad.sum()) == 5 + 51 + 55
        for buf in (self.flat.data, self.opt.velocity):
            buf[self.pad] = SENTINEL
        self.plan.copy[self.pad] = SENTINEL
        # float64 state
        self.p64 = self.flat.data.double().cpu()
        self.v64 = torch.zeros_like(self.p64)
        self.wd64 = torch.zeros_like(self.p64)
        for s in self.flat.segments:
            if len(s.shape) >= 2:
                self.wd64[s.offset:s.offset + s.numel] = f32(opt.get("weight_decay", 0.0))
        self.grads = []

    def close(self):
        N._PLANS.pop(id(self.flat), None)

    def new_grad(self):
        g = torch.randn(self.flat.total, generator=self.gen)
        g[self.pad.cpu()] = 0          # the padding carries no gradient
        self.flat.grad.copy_(g)
        self.grads.append(g)
        return g.double()

    def ref_step(self, g, factor, lr, momentum, nesterov):
        """One float64 step with the clip factor the device produced and the fp32 hyper-parameters the kernel reads."""
        lr, momentum = f32(lr), f32(momentum)
        ge = g * factor + self.wd64 * self.p64
        self.v64 = momentum * self.v64 - lr * ge
        self.p64 = self.p64 + momentum * self.v64 - lr * ge if nesterov else self.p64 + self.v64

    def check_state(self, p=None, v=None):
        """rtol 1e-5 plus an atol of 1e-6 x the buffer's largest reference magnitude, per element."""
        p = self.flat.data if p is None else p
        v = self.opt.velocity if v is None else v
        real = ~self.pad.cpu()
        for name, got, want in (("p", p, self.p64), ("v", v, self.v64)):
            atol = 1e-6 * float(want[real].abs().max())
            for s in self.flat.segments:
                a = slice(s.offset, s.offset + s.numel)
                err = (got[a].cpu().double() - want[a]).abs()
                bound = atol + 1e-5 * want[a].abs()
                print("{} {}: max error {:.3e}, smallest bound {:.3e}".format(name, s.shape, float(err.max()),
                                                                              float(bound.min())))
                assert bool((err <= bound).all()), (name, s.shape, float((err - bound).max()))

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
        for name, buf in (("data", self.flat.data), ("velocity", self.opt.velocity), ("copy", self.plan.copy)):
            assert bool((buf[self.pad].float() == torch.tensor(SENTINEL).to(buf.dtype).float().item()).all()), name


@pytest.fixture
def make_setup(cuda):
    made = []

    def make(seed, **kw):
        made.append(Setup(cuda, seed, **kw))
        return made[-1]

    yield make
    for s in made:
        s.close()


# the gradient norm is about sqrt(45,393) = 213: clipnorm 0.5 is active in every step
CASES = {
    # clipnorm, nesterov, weight decay, learning rates, momenta
    "momentum": (0.5, False, 0.0, [1e-2] * 5, [0.9] * 5),
    "nesterov_decay": (0.5, True, 1e-2, [1e-2] * 5, [0.9] * 5),
    "plain": (0.0, False, 0.0, [1e-2] * 5, [0.0] * 5),
    "lr_change": (0.5, False, 0.0, [1e-2, 1e-2, 2.5e-3, 2.5e-3, 2.5e-3], [0.9] * 5),
    "momentum_change": (0.5, False, 0.0, [1e-2] * 5, [0.9, 0.9, 0.5, 0.5, 0.5]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sgd_steps(make_setup, case):
    clipnorm, nesterov, wd, lrs, moms = CASES[case]
    st = make_setup(seed=41, lr=lrs[0], momentum=moms[0], nesterov=nesterov, weight_decay=wd, clipnorm=clipnorm)
    assert st.opt._use_hip()
    assert (st.opt.seg_wd() is None) == (wd == 0.0)
    if wd:
        assert st.opt.seg_wd().tolist() == [f32(wd), 0.0, f32(wd), f32(wd), f32(wd)]
    st.check_copy()                             # as built (ComputeWeights.build -> mxr_refresh_copy)
    gen0 = st.plan.generation
    for lr, mom in zip(lrs, moms):
        g = st.new_grad()
        st.opt.lr, st.opt.momentum = lr, mom
        norm, factor = st.opt.norm_and_scale()          # what step() computes again from the same gradient
        ref_norm = math.sqrt(float((g * g).sum()))
        ref_factor = f32(clipnorm) / ref_norm if clipnorm > 0 and ref_norm >= clipnorm else 1.0
        assert abs(norm.item() - ref_norm) <= 1e-5 * ref_norm
        assert abs(factor.item() - ref_factor) <= 1e-5 * ref_factor
        assert (ref_factor != 1.0) == (clipnorm == 0.5)
        if clipnorm == 0.0:
            assert factor.item() == 1.0
        norm2 = st.opt.step()
        assert norm2.item() == norm.item()
        st.ref_step(g, float(factor.item()), lr, mom, nesterov)
        st.check_state()
        st.check_copy()
    assert st.opt.iterations == STEPS and st.plan.iter.item() == STEPS and st.plan.host_iter == STEPS
    assert st.plan.generation == gen0 + STEPS
    st.check_padding()
    assert st.plan.hyper[1].item() == f32(lrs[-1]) and st.plan.hyper[2].item() == f32(moms[-1])


@pytest.mark.parametrize("case", ["momentum", "nesterov_decay"])
def test_hip_against_torch_backend(make_setup, case):
    clipnorm, nesterov, wd, lrs, moms = CASES[case]
    kw = dict(lr=lrs[0], momentum=moms[0], nesterov=nesterov, weight_decay=wd, clipnorm=clipnorm)
    hip = make_setup(seed=44, **kw)
    ref = make_setup(seed=44, backend="torch", **kw)
    assert hip.opt._use_hip() and not ref.opt._use_hip()
    assert torch.equal(hip.flat.data, ref.flat.data)
    for _ in range(STEPS):
        g = hip.new_grad()
        ref.flat.grad.copy_(hip.flat.grad)
        _, factor = hip.opt.norm_and_scale()
        hip.opt.step()
        ref.opt.step()
        hip.ref_step(g, float(factor.item()), lrs[0], moms[0], nesterov)
    # both against the same float64 run, within the same tolerance
    hip.check_state()
    hip.check_state(ref.flat.data, ref.opt.velocity)
    # and against each other
    real = ~hip.pad
    for name, a, b in (("p", hip.flat.data, ref.flat.data), ("v", hip.opt.velocity, ref.opt.velocity)):
        a, b = a[real].double(), b[real].double()
        bound = 1e-6 * float(b.abs().max()) + 1e-5 * b.abs()
        assert bool(((a - b).abs() <= bound).all()), (name, float(((a - b).abs() - bound).max()))
    assert ref.opt.iterations == hip.opt.iterations == STEPS
    hip.check_padding()
