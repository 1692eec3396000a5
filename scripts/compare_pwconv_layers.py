"""Layer by layer on the activations of the MobileNet(0.25) model tests (seed 5, bf16, 2 x 64 x 96): how many output
elements of the pointwise kernels (csrc/kernels/pwconv.hip) differ from F.conv2d on the same input, and the error of
each against the float64 product.  Output kept as profiles/pwconv_layers.txt.
python scripts/compare_pwconv_layers.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import pointwise as P

torch.manual_seed(5)
ref = MobileNet(0.25).double()
x = torch.randn(2, 64, 96, 3).bfloat16()
dev = torch.device("cuda:0")
m = MobileNet(0.25)
m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
m = m.to(dev)
m.pw_backend = "torch"
cap = {}
for i in range(13):
    m.pw[i].register_forward_hook(lambda mod, inp, out, i=i: cap.__setitem__(i, (inp[0].detach(), out.detach())))
with torch.no_grad():
    m(x.to(dev))
for i in range(13):
    xin, yt = cap[i]
    xh = xin.permute(0, 2, 3, 1)
    w = m.pw[i].weight.detach()
    yn = P.pointwise_conv(xh, w, "native").permute(0, 3, 1, 2)
    y64 = P.pointwise_conv_torch(xh.double().cpu(), w.bfloat16().double().cpu()).permute(0, 3, 1, 2)
    dn = (yn.double().cpu() - y64).abs()
    dt = (yt.double().cpu() - y64).abs()
    ne = int((yn != yt).sum())
    print("conv_pw_{:<2} {} -> {}, M {:5d}: elements differing {:6d} of {:7d}; max |err| vs float64: native {:.3e} torch {:.3e}; "
          "mean |err|: native {:.3e} torch {:.3e}".format(i + 1, w.shape[1], w.shape[0], xh.numel() // w.shape[1], ne, yn.numel(),
                                                        float(dn.max()), float(dt.max()), float(dn.mean()), float(dt.mean())))
