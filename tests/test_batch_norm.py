"""``ops.norm`` batch norm + activation on the CPU: the torch expression against a float64 loop over the channels (biased
batch variance for the output, unbiased for the running variance), and MobileNet's ``bn_backend`` switch."""
import copy

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import norm as norm_ops

EPS, MOM = 1e-3, 0.01
CLAMP = {"none": (-float("inf"), float("inf")), "relu": (0.0, float("inf")), "relu6": (0.0, 6.0)}


def channel_loop(x, gamma, beta, rmean, rvar, training, act):
    """(y, running_mean, running_var) channel by channel in float64; the running statistics are not modified."""
    y, rmean, rvar = torch.empty_like(x), rmean.clone(), rvar.clone()
    n = x.numel() // x.shape[3]
    for c in range(x.shape[3]):
        v = x[..., c]
        mean, var = rmean[c], rvar[c]
        if training:
            mean = v.sum() / n
            var = ((v - mean) ** 2).sum() / n
            rmean[c] = (1 - MOM) * rmean[c] + MOM * mean
            rvar[c] = (1 - MOM) * rvar[c] + MOM * var * n / (n - 1)
        y[..., c] = (gamma[c] * (v - mean) / torch.sqrt(var + EPS) + beta[c]).clamp(*CLAMP[act])
    return y, rmean, rvar


@pytest.mark.parametrize("act", ("none", "relu", "relu6"))
@pytest.mark.parametrize("training", (True, False))
def test_torch_expression_matches_channel_loop(training, act):
    g = torch.Generator().manual_seed(4)
    gamma, beta, rmean = (o + s * torch.randn(8, dtype=torch.float64, generator=g) for o, s in ((2, 0.5), (3, 1), (0, 1)))
    rvar = 0.5 + torch.rand(8, dtype=torch.float64, generator=g)
    want_m, want_v = rmean, rvar
    for _ in range(2):                               # two steps: the second starts from the updated statistics
        x = torch.randn(2, 3, 5, 8, dtype=torch.float64, generator=g)
        want, want_m, want_v = channel_loop(x, gamma, beta, want_m, want_v, training, act)
        y = norm_ops.batch_norm_act_torch(x, (gamma, beta, rmean, rvar), training, act, MOM, EPS)
        assert y.shape == x.shape and (y - want).abs().max() <= 1e-12
    assert (rmean - want_m).abs().max() <= 1e-13 and (rvar - want_v).abs().max() <= 1e-13
    if act == "relu6":
        assert bool((want == 0).any()) and bool((want == 6).any())


def test_mobilenet_backends_bit_equal_on_cpu():
    torch.manual_seed(0)
    base = MobileNet(0.25)
    x = torch.randn(2, 64, 96, 3)
    outs, states = {}, {}
    for backend in ("auto", "torch"):
        m = copy.deepcopy(base)
        m.bn_backend = backend
        outs[backend] = m(x)
        assert m.bn_taken == ["torch"] * 27
        states[backend] = m.state_dict()
    for a, b in zip(outs["auto"], outs["torch"]):
        assert torch.equal(a, b)
    assert list(states["auto"]) == list(base.state_dict())
    for k, v in states["auto"].items():
        assert torch.equal(v, states["torch"][k]), k
    assert int(states["auto"]["conv1_bn.bn.num_batches_tracked"]) == 1
