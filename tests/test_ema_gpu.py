"""The EMA forms of the fused optimizer kernels (``mxr_adam_step_ema`` / ``mxr_sgd_step_ema``) and ``mxr_swap_refresh``
(csrc/kernels/optim.hip) over the segments of tests/test_sgd_gpu.py: rows that straddle 4-vectors, a scalar tail,
segments that cross chunks (AdamPlan.CHUNK = 8192) with a 9-element last chunk, and exactly full chunks.  The EMA
arithmetic is isolated: the float64 oracle averages the device's own weights with the fp32 decay of each update, which
the device must also have produced (``hyper[3]``).  A twin run without the EMA must stay bit-identical in everything
else.  Every padding element of the flat layout carries a sentinel."""
import numpy as np
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.train.flat import FlatParams
from batchai_retinanet_horovod_coco_amd.train.optimizer import KerasAdam, KerasSGD

pytestmark = pytest.mark.gpu

# shape, has a per-output-channel scale
PARAMS = [
    ((7, 3, 3, 5), True),      # row length 45: 4-vectors straddle rows
    ((13,), False),            # three vectors and a scalar tail
    ((64, 1, 1, 64), True),
    ((3, 8195), True),         # 24,585 = 3 x 8192 + 9: a last chunk of two vectors and a scalar tail
    ((2, 8192), False),        # exactly two whole chunks
]
SENTINEL = -12345.0
EMA_SENTINEL = -54321.0        # another one for the average's padding: an exchange of padding would show
D = 0.5                        # the ramp (1 + n) / (10 + n) reaches it at n = 8: both branches of the min run

# the gradient norm is about sqrt(45,393) = 213: clipnorm 0.5 is active in every step
CASES = {
    "adam": (KerasAdam, dict(lr=1e-3, clipnorm=0.5)),
    "sgd_momentum": (KerasSGD, dict(lr=1e-2, momentum=0.9, clipnorm=0.5)),
    "sgd_nesterov_decay": (KerasSGD, dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-2, clipnorm=0.5)),
}


def ramp(n, cap=D):
    return float(min(np.float32(cap), np.float32(1 + n) / np.float32(10 + n)))


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
    def __init__(self, dev, seed, case, ema_decay, backend="auto"):
        gen = torch.Generator().manual_seed(seed)
        self.gen = gen
        self.params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s, _ in PARAMS]
        self.scales = [(torch.rand(s[0], generator=gen) + 0.5).to(dev) if sc else None for s, sc in PARAMS]
        self.flat = FlatParams([(str(i), p) for i, p in enumerate(self.params)])
        # registers its AdamPlan (copy=True, scales) for this flat buffer: the steps below use it
        self.cw = N.ComputeWeights(self.flat, [_Conv(p, s) for p, s in zip(self.params, self.scales)])
        self.plan = self.cw.plan
        assert N.adam_plan(self.flat) is self.plan and self.plan.copy is not None
        assert self.plan.nchunks == 1 + 1 + 1 + 4 + 2
        cls, kw = CASES[case]
        self.opt = cls(self.flat, backend=backend, ema_decay=ema_decay, **kw)
        self.pad = torch.ones(self.flat.total, dtype=torch.bool, device=dev)
        for s in self.flat.segments:
            self.pad[s.offset:s.offset + s.numel] = False
        assert int(self.pad.sum()) == 5 + 51 + 55
        self.slots = {k: v for k, v in self.opt.state_tensors().items() if k != "ema"}
        for buf in [self.flat.data] + list(self.slots.values()):
            buf[self.pad] = SENTINEL
        self.plan.copy[self.pad] = SENTINEL
        if self.opt.ema is not None:
            assert torch.equal(self.opt.ema[~self.pad], self.flat.data[~self.pad])      # seeded with the weights
            self.opt.ema[self.pad] = EMA_SENTINEL
            self.ema64 = self.opt.ema.double()

    def close(self):
        N._PLANS.pop(id(self.flat), None)

    def new_grad(self, *others):
        g = torch.randn(self.flat.total, generator=self.gen)
        g[self.pad.cpu()] = 0          # the padding carries no gradient
        for st in (self,) + others:
            st.flat.grad.copy_(g)

    def ref_ema(self, d):
        """The EMA arithmetic alone: float64, over the device's own weights after the step, with the fp32 decay."""
        self.ema64 = d * self.ema64 + (1.0 - d) * self.flat.data.double()

    def check_ema(self, got=None, what="ema"):
        """The project's per-element bound: 1e-5 |ref| + 1e-6 max |ref| (a convex combination: no cancellation)."""
        got = self.opt.ema if got is None else got
        real = ~self.pad
        want = self.ema64[real]
        err = (got[real].double() - want).abs()
        bound = 1e-5 * want.abs() + 1e-6 * float(want.abs().max())
        print("{}: max error {:.3e}, smallest bound {:.3e}".format(what, float(err.max()), float(bound.min())))
        assert bool((err <= bound).all()), (what, float((err - bound).max()))

    def check_copy(self):
        """Every compute copy is exactly bf16(p * scale of its output channel)."""
        for s, sc in zip(self.flat.segments, self.scales):
            p = self.flat.data[s.offset:s.offset + s.numel].view(s.shape[0], -1)
            want = (p * sc[:, None] if sc is not None else p).bfloat16().reshape(-1)
            got = self.plan.copy[s.offset:s.offset + s.numel]
            bad = (got != want).nonzero().flatten()
            assert bad.numel() == 0, "compute copy of segment {} (row length {}): {} elements differ, first at {}".format(
                s.shape, s.numel // s.shape[0], bad.numel(), bad[:8].tolist())

    def check_padding(self):
        bufs = [("data", self.flat.data, SENTINEL), ("copy", self.plan.copy, SENTINEL)]
        bufs += [(k, v, SENTINEL) for k, v in self.slots.items()]
        if self.opt.ema is not None:
            bufs.append(("ema", self.opt.ema, EMA_SENTINEL))
        for name, buf, val in bufs:
            assert bool((buf[self.pad].float() == torch.tensor(val).to(buf.dtype).float().item()).all()), name


@pytest.fixture
def make_setup(cuda):
    made = []

    def make(seed, case, ema_decay, **kw):
        made.append(Setup(cuda, seed, case, ema_decay, **kw))
        return made[-1]

    yield make
    for s in made:
        s.close()


@pytest.mark.parametrize("case", ["adam", "sgd_momentum", "sgd_nesterov_decay"])
def test_ema_steps(make_setup, case):
    st = make_setup(41, case, D)
    twin = make_setup(41, case, 0.0)            # the same run without the average
    assert st.opt._use_hip() and twin.opt._use_hip() and twin.opt.ema is None
    assert torch.equal(st.flat.data, twin.flat.data)
    gen0 = st.plan.generation
    for n in range(1, 13):
        st.new_grad(twin)
        st.opt.step()
        twin.opt.step()
        d = ramp(n)
        assert st.plan.hyper[3].item() == d == st.opt.ema_decay_at(n), (n, st.plan.hyper[3].item(), d)
        assert st.opt.ema_updates == n
        st.ref_ema(d)
        st.check_ema(what="ema after update {}".format(n))
        # the fused forms change nothing else
        assert torch.equal(st.flat.data, twin.flat.data), n
        for k in st.slots:
            assert torch.equal(st.slots[k], twin.slots[k]), (k, n)
        assert torch.equal(st.plan.copy, twin.plan.copy), n
    st.check_copy()
    st.check_padding()
    twin.check_padding()
    assert twin.plan.hyper[3].item() == 0.0
    assert st.plan.iter.item() == st.plan.host_iter == st.opt.iterations == 12
    assert st.plan.generation == gen0 + 12
    assert not torch.equal(st.opt.ema[~st.pad], st.flat.data[~st.pad])


def test_ema_start_offset(make_setup):
    st = make_setup(43, "sgd_momentum", D)
    # as a restore sets them: 7 steps done, the average seeded at step 4 and updated 3 times
    st.opt.iterations, st.opt.ema_start = 7, 4
    assert st.opt.ema_updates == 3
    e = torch.randn(st.flat.total, generator=st.gen).to(st.flat.data.device)
    st.opt.ema[~st.pad] = e[~st.pad]
    st.ema64 = st.opt.ema.double()
    st.new_grad()
    st.opt.step()
    d4 = ramp(4)
    assert d4 == float(np.float32(5) / np.float32(14)) and d4 != ramp(8)     # not the step count's d_8
    assert st.plan.hyper[3].item() == d4
    st.ref_ema(d4)
    st.check_ema()
    assert st.opt.ema_updates == 4 and st.plan.iter.item() == st.plan.host_iter == st.opt.iterations == 8
    st.check_padding()


@pytest.mark.parametrize("case", ["adam", "sgd_momentum"])
def test_hip_against_torch_backend(make_setup, case):
    hip = make_setup(44, case, D)
    ref = make_setup(44, case, D, backend="torch")
    assert hip.opt._use_hip() and not ref.opt._use_hip()
    for n in range(1, 6):
        hip.new_grad(ref)
        hip.opt.step()
        ref.opt.step()
        hip.ref_ema(ramp(n))
        ref.ref_ema(ramp(n))
    hip.check_ema()
    ref.check_ema()
    # and the kernel's average against the torch backend's
    hip.ema64 = ref.opt.ema.double()
    hip.check_ema(what="hip against torch")
    assert hip.opt.ema_updates == ref.opt.ema_updates == 5
    hip.check_padding()


def test_swap_refresh(make_setup):
    st = make_setup(45, "sgd_momentum", D)
    for _ in range(2):
        st.new_grad()
        st.opt.step()
    p0, e0 = st.flat.data.clone(), st.opt.ema.clone()
    real = ~st.pad
    assert not torch.equal(p0[real], e0[real])
    ptrs = (st.flat.data.data_ptr(), st.opt.ema.data_ptr(), st.plan.copy.data_ptr())
    gen0 = st.plan.generation
    N.swap_refresh(st.flat, st.opt.ema)
    assert st.plan.generation == gen0 + 1
    assert torch.equal(st.flat.data[real], e0[real]) and torch.equal(st.opt.ema[real], p0[real])
    st.check_copy()                 # of the averaged weights now in place
    st.check_padding()              # each buffer's own sentinel: the padding was not exchanged
    N.swap_refresh(st.flat, st.opt.ema)
    assert st.plan.generation == gen0 + 2
    assert torch.equal(st.flat.data, p0) and torch.equal(st.opt.ema, e0)
    st.check_copy()
    st.check_padding()
    assert ptrs == (st.flat.data.data_ptr(), st.opt.ema.data_ptr(), st.plan.copy.data_ptr())
    assert st.plan.iter.item() == st.opt.iterations == 2
