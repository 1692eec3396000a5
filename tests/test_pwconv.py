"""``ops.pointwise`` without a GPU: the torch expression against a plain matrix product, the backend switch, and
MobileNet's ``pw_backend`` wiring."""
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import pointwise as P


@pytest.mark.parametrize("nhw,ci,co", (((1, 1, 1), 8, 8), ((2, 3, 5), 12, 7), ((1, 4, 2), 3, 16)))
def test_torch_expression_is_the_matrix_product(nhw, ci, co):
    g = torch.Generator().manual_seed(ci + co)
    x = torch.randn(*nhw, ci, generator=g, dtype=torch.float64)
    w = torch.randn(co, ci, 1, 1, generator=g, dtype=torch.float64)
    y = P.pointwise_conv_torch(x, w)
    assert tuple(y.shape) == nhw + (co,)
    want = (x.reshape(-1, ci) @ w.reshape(co, ci).t()).reshape(*nhw, co)
    assert torch.allclose(y, want, rtol=1e-13, atol=1e-13)


def test_backends_on_cpu():
    x, w = torch.randn(1, 2, 3, 8), torch.randn(16, 8, 1, 1)
    assert not P.takes_native(x, 16)
    assert torch.equal(P.pointwise_conv(x, w), P.pointwise_conv_torch(x, w))
    with pytest.raises(RuntimeError, match="needs a GPU tensor"):
        P.pointwise_conv(x, w, backend="native")
    with pytest.raises(ValueError):
        P.pointwise_conv(x, w, backend="hip")


def test_mobilenet_auto_is_torch_on_cpu():
    torch.manual_seed(3)
    m = MobileNet(0.25).eval()
    x = torch.randn(1, 64, 96, 3)
    m.pw_backend = "auto"
    with torch.no_grad():
        auto = m(x)
        assert m.pw_taken == ["torch"] * 13
        m.pw_backend = "torch"
        plain = m(x)
    assert m.pw_taken == ["torch"] * 13
    assert all(torch.equal(a, b) for a, b in zip(auto, plain))
