"""The separable block's torch expression and MobileNet's ``block_backend`` switch on the CPU."""
import pytest
import torch
import torch.nn.functional as F

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import separable as SB


def randomise_statistics(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 3.75 + 0.25)


@pytest.mark.parametrize("i", (0, 1))        # block 1 has stride 1, block 2 stride 2
def test_torch_expression_is_the_four_modules(i):
    torch.manual_seed(3)
    m = MobileNet(0.25).eval()
    randomise_statistics(m, 4)
    s, ci = m.strides[i], m.dw[i].weight.shape[0]
    x = torch.randn(2, 9, 14, ci)
    with torch.no_grad():
        z = x.permute(0, 3, 1, 2)
        z = F.pad(z, (1, 1, 1, 1)) if s == 1 else F.pad(z, (0, 1, 0, 1))
        want = m.pw_bn[i](m.pw[i](m.dw_bn[i](m.dw[i](z)))).permute(0, 2, 3, 1)
        got = SB.separable_block_eval_torch(x, m.dw[i].weight, m.dw_bn[i].bn, m.pw[i].weight, m.pw_bn[i].bn, s)
        assert torch.equal(got, SB.separable_block_eval(x, m.dw[i].weight, m.dw_bn[i].bn, m.pw[i].weight,
                                                        m.pw_bn[i].bn, s))
    assert got.shape == ((2, 9, 14) if s == 1 else (2, 4, 7)) + (m.pw[i].weight.shape[0],)
    assert torch.equal(got, want)


def test_block_backend_on_cpu():
    torch.manual_seed(4)
    m = MobileNet(0.25).eval()
    randomise_statistics(m, 5)
    assert m.block_backend == "torch"
    x = torch.randn(1, 64, 96, 3)
    with torch.no_grad():
        want = m(x)
        assert m.block_taken == ["layers"] * 13
        m.block_backend = "auto"
        got = m(x)
        assert m.block_taken == ["layers"] * 13 and len(m.dw_taken) == 13 and len(m.bn_taken) == 27
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        m.block_backend = "native"
        with pytest.raises(RuntimeError):
            m(x)
        with pytest.raises(RuntimeError):
            SB.separable_block_eval(torch.randn(1, 4, 4, 8), m.dw[0].weight, m.dw_bn[0].bn, m.pw[0].weight,
                                    m.pw_bn[0].bn, 1, backend="native")
        m.block_backend = "hip"
        with pytest.raises(ValueError):
            m(x)
        with pytest.raises(ValueError):
            SB.separable_block_eval(torch.randn(1, 4, 4, 8), m.dw[0].weight, m.dw_bn[0].bn, m.pw[0].weight,
                                    m.pw_bn[0].bn, 1, backend="hip")


def test_training_mode_takes_no_fused_block():
    torch.manual_seed(6)
    m = MobileNet(0.25).train()
    m.block_backend = "auto"
    m(torch.randn(2, 32, 32, 3))
    assert m.block_taken == ["layers"] * 13
    m.block_backend = "native"          # the switch is for eval mode: a training forward runs the layers
    m(torch.randn(2, 32, 32, 3))
    assert m.block_taken == ["layers"] * 13
