"""What stem_backend = "auto" would do to the three MobileNet(0.25) model tests (test_mobilenet_native_against_float64 in
tests/test_dwconv_gpu.py, test_batch_norm_gpu.py and test_pwconv_gpu.py; seed 5, bf16, 2 x 64 x 96): for each test's
switch (dw / bn / pw backend 'torch' against 'native', the others at their defaults) and each stem backend, max |dev| /
max |ref| of C3..C5 against the float64 CPU run, and whether the tests' rule (native <= 2 x torch) would hold.  First:
how many elements of the stem's output differ between the kernel and the torch expression on that image.  Output kept
as profiles/stem3x3_models.txt.
python scripts/compare_stem3x3_models.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import stem3x3 as S3

torch.manual_seed(5)
ref = MobileNet(0.25).double()
x = torch.randn(2, 64, 96, 3).bfloat16()
dev = torch.device("cuda:0")
state = {k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()}
want = [o.detach() for o in ref(x.double())]

w = state["conv1.weight"].to(dev)
yn = S3.stem_conv3x3(x.to(dev), w, "native")
yt = S3.stem_conv3x3_torch(x.to(dev), w.bfloat16())
y64 = S3.stem_conv3x3_torch(x.double(), w.bfloat16().double().cpu())
print("conv1 3 -> 8, M {}: elements differing {} of {}; max |err| vs float64: native {:.3e} torch {:.3e}".format(
    yn.numel() // 8, int((yn != yt).sum()), yn.numel(), float((yn.double().cpu() - y64).abs().max()),
    float((yt.double().cpu() - y64).abs().max())))

for attr in ("dw_backend", "bn_backend", "pw_backend"):
    for stem in ("torch", "auto"):
        devs = {}
        for backend in ("torch", "native"):
            m = MobileNet(0.25)
            m.load_state_dict(state)
            for b in [m.conv1_bn] + list(m.dw_bn) + list(m.pw_bn):
                b.bn.reset_running_stats()
            setattr(m, attr, backend)
            m.stem_backend = stem
            with torch.no_grad():
                got = m.to(dev)(x.to(dev))
            devs[backend] = [float((g.double().cpu() - r).abs().max() / r.abs().max()) for g, r in zip(got, want)]
        print("{} torch / native, stem_backend {:<5} (conv1 ran as {:<6}): ".format(attr, stem, m.stem_taken) + "  ".join(
            "{} {:.3e} / {:.3e} ({})".format(n, t, nat, "holds" if nat <= 2.0 * t else "BREAKS")
            for n, t, nat in zip(("C3", "C4", "C5"), devs["torch"], devs["native"])))
