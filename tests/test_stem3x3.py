"""The stem conv's torch expression and MobileNet's ``stem_backend`` switch on the CPU."""
import pytest
import torch
import torch.nn.functional as F

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import stem3x3 as S3


@pytest.mark.parametrize("hw", ((2, 2), (9, 14), (8, 13), (32, 48)))
def test_torch_expression_is_pad_and_conv1(hw):
    torch.manual_seed(3)
    m = MobileNet(0.25)
    x = torch.randn(2, *hw, 3)
    want = m.conv1(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1))).permute(0, 2, 3, 1)
    got = S3.stem_conv3x3_torch(x, m.conv1.weight)
    assert got.shape == (2, (hw[0] - 2) // 2 + 1, (hw[1] - 2) // 2 + 1, 8)
    assert torch.equal(got, want)


def test_stem_backend_on_cpu():
    torch.manual_seed(4)
    m = MobileNet(0.25)
    assert m.stem_backend == "torch"
    x = torch.randn(1, 64, 96, 3)
    want = [o.detach() for o in m(x)]
    assert m.stem_taken == "torch"
    m.stem_backend = "auto"
    got = m(x)
    assert m.stem_taken == "torch"
    assert all(torch.equal(a.detach(), b) for a, b in zip(got, want))
    m.stem_backend = "native"
    with pytest.raises(RuntimeError):
        m(x)
    with pytest.raises(RuntimeError):
        S3.stem_conv3x3(x, m.conv1.weight, backend="native")
    m.stem_backend = "hip"
    with pytest.raises(ValueError):
        m(x)
    with pytest.raises(ValueError):
        S3.stem_conv3x3(x, m.conv1.weight, backend="hip")
