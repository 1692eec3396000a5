"""``ops.depthwise`` on the CPU: the torch expression against a float64 loop over taps (Keras padding: one pixel on every
side at stride 1, bottom and right only at stride 2), the CPU dispatch, and MobileNet's ``dw_backend`` switch."""
import warnings

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import depthwise as D


def taps_loop(x, w, stride):
    """y[n, oy, ox, c] = sum x[n, oy s + ky - pad, ox s + kx - pad, c] w[c, 0, ky, kx], taps outside reading zero."""
    N, H, W, C = x.shape
    pad = 1 if stride == 1 else 0
    Ho, Wo = (H, W) if stride == 1 else ((H - 2) // 2 + 1, (W - 2) // 2 + 1)
    y = torch.zeros(N, Ho, Wo, C, dtype=torch.float64)
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
                    if 0 <= iy < H and 0 <= ix < W:
                        y[:, oy, ox] += x[:, iy, ix] * w[:, 0, ky, kx]
    return y


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("shape", ((2, 5, 4, 8), (1, 4, 5, 8)))
def test_torch_expression_matches_tap_loop(shape, stride):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, dtype=torch.float64, generator=g)
    w = torch.randn(shape[3], 1, 3, 3, dtype=torch.float64, generator=g)
    ref = taps_loop(x, w, stride)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = D.depthwise_conv3x3(x, w, stride)        # the CPU takes the torch path, silently
    assert y.shape == ref.shape
    assert (y - ref).abs().max() <= 1e-13
    assert torch.equal(y, D.depthwise_conv3x3(x, w, stride, backend="torch"))


def test_native_backend_raises_on_cpu():
    x, w = torch.randn(1, 4, 4, 8), torch.randn(8, 1, 3, 3)
    with pytest.raises(RuntimeError):
        D.depthwise_conv3x3(x, w, 1, backend="native")


def test_mobilenet_backends_bit_equal_on_cpu():
    torch.manual_seed(0)
    m = MobileNet(0.25)
    x = torch.randn(2, 64, 96, 3)
    outs = {}
    for backend in ("auto", "torch"):
        m.dw_backend = backend
        torch.manual_seed(1)
        outs[backend] = m(x)
        assert m.dw_taken == ["torch"] * 13
    for a, b in zip(outs["auto"], outs["torch"]):
        assert torch.equal(a, b)
