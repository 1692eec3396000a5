"""The rule that picks the separable block's kernel form, and the CPU path of a block wide enough for the stream form."""
import torch

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops import separable as SB


def test_form_rule_on_mobilenet_and_the_tested_resident_shapes():
    forms = [N.sepblock_form(ci, co) for ci, co in zip([32] + MobileNet.FILTERS[:-1], MobileNet.FILTERS)]
    assert forms == ["resident"] * 6 + ["stream"] * 7
    assert N.sepblock_form(264, 16) == "resident" and N.sepblock_form(264, 256) == "stream"
    assert N.sepblock_form(256, 512) == "resident"


def test_cpu_block_with_264_channels_is_the_torch_expression():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 5, 7, 264, generator=g)
    wdw, wpw = torch.randn(264, 1, 3, 3, generator=g), torch.randn(256, 264, 1, 1, generator=g)
    bn1, bn2 = torch.nn.BatchNorm2d(264).eval(), torch.nn.BatchNorm2d(256).eval()
    for bn in (bn1, bn2):
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
    with torch.no_grad():
        for s in (1, 2):
            assert torch.equal(SB.separable_block_eval(x, wdw, bn1, wpw, bn2, s),
                               SB.separable_block_eval_torch(x, wdw, bn1, wpw, bn2, s))
