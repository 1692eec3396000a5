"""Experimental backbones of the keras-retinanet registry: VGG16/19, MobileNet (v1), DenseNet.

The reference accepts any registered backbone name (``--backbone``, ``/root/reference/train.py:364``)
and warns that only ResNet-50 is properly tested (``train.py:323-324``); for vgg/densenet it
measures the real pyramid shapes with ``make_shapes_callback(model)`` (``train.py:428-432``).
Layer names follow keras.applications so ``--weights`` by-name loading lines up:

* VGG16/19: ``block{b}_conv{i}`` (3x3 same + bias + ReLU), ``block{b}_pool``; C3..C5 =
  block3_pool / block4_pool / block5_pool;
* MobileNet(alpha): ``conv1`` 3x3/s2 + ``conv1_bn``, 13 depthwise-separable blocks
  ``conv_dw_{i}`` / ``conv_pw_{i}`` (+ ``_bn``, ReLU6); C3..C5 = conv_pw_5/11/13 outputs;
* DenseNet121/169/201: ``conv1/conv`` 7x7/s2, pool, dense blocks ``conv{s}_block{i}`` (BN-ReLU-1x1
  (4k)-BN-ReLU-3x3(k), concat), transitions ``pool{s}`` (BN-ReLU-1x1, avg-pool 2); C3..C5 = the
  outputs of dense blocks 2, 3, 4.

As in keras.applications, BN in MobileNet/DenseNet is ordinary (trainable, batch statistics in
training).  VGG convs run through the same conv front-end as ResNet (HIP implicit GEMM when the
shape class is covered).  MobileNet's 13 depthwise 3x3 convs run on the HIP kernels of ``csrc/kernels/dwconv.hip``
(``ops.depthwise``) and its 27 batch-norms + ReLU6 on those of ``csrc/kernels/batch_norm.hip`` (``ops.norm``) for bf16
activations on the GPU; its 13 pointwise 1x1 convs run on the MFMA kernels of ``csrc/kernels/pwconv.hip``
(``ops.pointwise``) when ``pw_backend`` is set to ``auto`` or ``native`` and as PyTorch/MIOpen ops by default; its stem
(3x3 / s2 on 3 channels) runs on the MFMA kernels of ``csrc/kernels/stem3x3.hip`` (``ops.stem3x3``), straight from the
NHWC image with the padding inside the kernel, when ``stem_backend`` is set to ``auto`` or ``native`` and as pad +
PyTorch/MIOpen conv + channels-last copy by default.  When the model is not training and ``block_backend`` is set to
``auto`` or ``native``, each of the 13 blocks (depthwise conv, norm, pointwise conv, norm) runs as one launch of
``csrc/kernels/sepblock.hip`` or, for the wide blocks (``Ci > 256``), of its K-streamed form
``csrc/kernels/sepblock_stream.hip`` (``ops.separable``) instead of its four layers.  All of DenseNet (which concatenates in NCHW) uses PyTorch/MIOpen
ops.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import depthwise as dw_ops
from ..ops import norm as norm_ops
from ..ops import pointwise as pw_ops
from ..ops import separable as sep_ops
from ..ops import stem3x3 as stem_ops
from .layers import Conv2D


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _bn_weights(name, bnact):
    b = bnact.bn
    return [(name + "/gamma:0", b.weight, "plain"), (name + "/beta:0", b.bias, "plain"),
            (name + "/moving_mean:0", b.running_mean, "plain"), (name + "/moving_variance:0", b.running_var, "plain")]


def _autocast(x):
    """Run torch-op backbones in the trainer's compute dtype (BN statistics stay fp32)."""
    return torch.autocast(device_type=x.device.type, dtype=x.dtype, enabled=x.dtype != torch.float32)


class _ShapeProbe:
    """Pyramid shapes measured with a real (no-grad) forward, cached per input size."""

    def feature_shapes_probe(self, image_hw: Sequence[int]) -> List[Tuple[int, int]]:
        key = (int(image_hw[0]), int(image_hw[1]))
        cache = self.__dict__.setdefault("_shape_cache", {})
        if key not in cache:
            p = next(self.parameters())
            with torch.no_grad():
                x = torch.zeros((1, key[0], key[1], 3), device=p.device, dtype=torch.float32)
                was = self.training
                self.eval()
                outs = self(x)
                self.train(was)
            cache[key] = [(int(o.shape[1]), int(o.shape[2])) for o in outs]
        return cache[key]


class VGG(nn.Module, _ShapeProbe):
    CFG = {"vgg16": [2, 2, 3, 3, 3], "vgg19": [2, 2, 4, 4, 4]}

    def __init__(self, name: str = "vgg16"):
        super().__init__()
        self.name = name
        widths = [64, 128, 256, 512, 512]
        blocks = []
        cin = 3
        for b, (n, w) in enumerate(zip(self.CFG[name], widths)):
            layers = nn.ModuleList()
            for i in range(n):
                layers.append(Conv2D("block{}_conv{}".format(b + 1, i + 1), cin, w, 3, 1, "same", True, True,
                                     "glorot_uniform"))
                cin = w
            blocks.append(layers)
        self.blocks = nn.ModuleList(blocks)
        self.out_channels = [128, 256, 512, 512]

    def forward(self, x):
        outs = []
        for b, layers in enumerate(self.blocks):
            for c in layers:
                x = c(x)
            x = _nhwc(F.max_pool2d(_nchw(x), 2, 2))
            if b >= 2:
                outs.append(x)
        return outs

    def convs(self):
        return [c for layers in self.blocks for c in layers]

    def keras_layers(self):
        return [(c.keras_name, [(c.keras_name + "/kernel:0", c.weight, "kernel"),
                                (c.keras_name + "/bias:0", c.bias, "plain")]) for c in self.convs()]

    def feature_shapes(self, image_hw):
        h, w = image_hw
        shapes = []
        for b in range(5):
            h, w = h // 2, w // 2
            shapes.append((h, w))
        return [shapes[0]] + shapes[2:5]


class _BNAct(nn.Module):
    def __init__(self, c, act="relu", eps=1e-3, momentum=0.01):
        super().__init__()
        self.bn = nn.BatchNorm2d(c, eps=eps, momentum=momentum)
        self.act = act

    def forward(self, x, backend="torch", taken=None):    # NCHW
        """``backend`` other than 'torch': the kernels of batch_norm.hip on the NHWC view where they serve it (no copy
        once ``x`` is channels-last); ``self.bn`` stays the holder of parameters and buffers.  ``taken`` collects the
        path."""
        xh = x.permute(0, 2, 3, 1)
        native = backend == "native" or norm_ops.bn_takes_native(xh, self.bn.training, backend)
        if taken is not None:
            taken.append("native" if native else "torch")
        if native:
            y = norm_ops.batch_norm_act(xh, self.bn, self.bn.training, self.act, backend)
            if self.bn.training:
                self.bn.num_batches_tracked.add_(1)      # on the device, as nn.BatchNorm2d does
            return _nchw(y)
        x = self.bn(x)
        if self.act == "relu6":
            return F.relu6(x)
        if self.act == "relu":
            return F.relu(x)
        return x


class MobileNet(nn.Module, _ShapeProbe):
    STRIDES = [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]
    FILTERS = [64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024]

    def __init__(self, alpha: float = 1.0):
        super().__init__()
        c = int(32 * alpha)
        self.conv1 = nn.Conv2d(3, c, 3, 2, 0, bias=False)
        self.conv1_bn = _BNAct(c, "relu6")
        self.dw, self.dw_bn, self.pw, self.pw_bn, self.strides = (nn.ModuleList(), nn.ModuleList(), nn.ModuleList(),
                                                                   nn.ModuleList(), [])
        for s, f in zip(self.STRIDES, self.FILTERS):
            f = int(f * alpha)
            self.dw.append(nn.Conv2d(c, c, 3, s, 0, groups=c, bias=False))
            self.dw_bn.append(_BNAct(c, "relu6"))
            self.pw.append(nn.Conv2d(c, f, 1, 1, 0, bias=False))
            self.pw_bn.append(_BNAct(f, "relu6"))
            self.strides.append(s)
            c = f
        self.out_channels = [0, int(256 * alpha), int(512 * alpha), int(1024 * alpha)]
        # 'auto': dwconv.hip where it serves the layer (bf16 on the GPU), else the torch ops; 'torch': the torch ops;
        # 'native': the kernels or an error
        self.dw_backend = "auto"
        self.dw_taken = []       # per layer of the last forward: 'native' or 'torch'
        # the same three for batch_norm.hip, and the path of the 27 norms in forward order (the layer timings behind
        # 'auto' are profiles/batchnorm.txt)
        self.bn_backend = "auto"
        self.bn_taken = []
        # the same three for pwconv.hip and the 13 conv_pw layers (profiles/pwconv.txt), but 'torch' by default: the
        # kernels are opt-in ('auto' or 'native'), see the README
        self.pw_backend = "torch"
        self.pw_taken = []
        # the same three for stem3x3.hip and conv1 (profiles/stem3x3.txt), 'torch' by default as well; the path of the
        # last forward: 'native' or 'torch'
        self.stem_backend = "torch"
        self.stem_taken = None
        # the same three for sepblock.hip, which runs a whole block (conv_dw, its norm, conv_pw, its norm) as one launch
        # when the model is not training (profiles/sepblock.txt; blocks 7 to 13 on sepblock_stream.hip,
        # profiles/sepblock_stream.txt); 'torch' by default: the four layers.  Per block of the last forward: 'fused'
        # (either kernel form) or 'layers'
        self.block_backend = "torch"
        self.block_taken = []

    def _block(self, i, x):
        """Block ``i + 1`` on NCHW ``x`` in one launch (eval mode only), or ``None`` where the four layers are to run;
        the modules stay the holders of every parameter and buffer."""
        if self.block_backend not in ("auto", "native", "torch"):
            raise ValueError("MobileNet.block_backend: 'auto', 'native' or 'torch' expected, got {!r}".format(
                self.block_backend))
        if self.training or self.block_backend == "torch":
            return None
        xh = x.permute(0, 2, 3, 1)
        ops = (xh, self.dw[i].weight, self.dw_bn[i].bn, self.pw[i].weight, self.pw_bn[i].bn, self.strides[i])
        if self.block_backend == "native" or sep_ops.takes_native(*ops, self.block_backend):
            return _nchw(sep_ops.separable_block_eval(*ops, self.block_backend))
        return None

    def _depthwise(self, i, x):
        """conv_dw_{i+1} on NCHW ``x``: the kernels on its NHWC view (no pad, no copy once ``x`` is channels-last), or
        the torch ops."""
        s = self.strides[i]
        xh = x.permute(0, 2, 3, 1)
        if self.dw_backend == "native" or dw_ops.takes_native(xh, s, self.dw_backend):
            self.dw_taken.append("native")
            return _nchw(dw_ops.depthwise_conv3x3(xh, self.dw[i].weight, s, self.dw_backend))
        self.dw_taken.append("torch")
        x = F.pad(x, (1, 1, 1, 1)) if s == 1 else F.pad(x, (0, 1, 0, 1))
        return self.dw[i](x)

    def _pointwise(self, i, x):
        """conv_pw_{i+1} on NCHW ``x``: the kernels on its NHWC view (no copy once ``x`` is channels-last), or the torch
        module; ``self.pw[i]`` stays the holder of the parameter."""
        xh = x.permute(0, 2, 3, 1)
        w = self.pw[i].weight
        if self.pw_backend == "native" or pw_ops.takes_native(xh, w.shape[0], self.pw_backend):
            self.pw_taken.append("native")
            return _nchw(pw_ops.pointwise_conv(xh, w, self.pw_backend))
        self.pw_taken.append("torch")
        return self.pw[i](x)

    def _stem(self, x):
        """conv1 on the NHWC image, NCHW out: the kernels (padding inside, NHWC result, so the view returned is already
        channels-last), or pad + the torch module; ``self.conv1`` stays the holder of the parameter."""
        if self.stem_backend not in ("auto", "native", "torch"):
            raise ValueError("MobileNet.stem_backend: 'auto', 'native' or 'torch' expected, got {!r}".format(
                self.stem_backend))
        w = self.conv1.weight
        if self.stem_backend == "native" or stem_ops.takes_native(x, w.shape[0], self.stem_backend):
            self.stem_taken = "native"
            return _nchw(stem_ops.stem_conv3x3(x, w, self.stem_backend))
        self.stem_taken = "torch"
        x = F.pad(_nchw(x), (0, 1, 0, 1))                # keras: ZeroPadding2D(((0,1),(0,1))) + valid s2
        return self.conv1(x)

    def forward(self, x):
        dt = x.dtype
        self.dw_taken, self.bn_taken, self.pw_taken, self.block_taken = [], [], [], []
        bn = (self.bn_backend, self.bn_taken)
        with _autocast(x):
            x = self._stem(x)
            xh = x.permute(0, 2, 3, 1)
            if self.bn_backend == "native" or norm_ops.bn_takes_native(xh, self.training, self.bn_backend):
                # once, in front of the first norm: all 27 are served on NHWC views that are no copies
                x = x.contiguous(memory_format=torch.channels_last)
            x = self.conv1_bn(x, *bn)
            if self.dw_backend == "native" or dw_ops.takes_native(x.permute(0, 2, 3, 1), 1, self.dw_backend):
                # once: BN, ReLU6 and the 1x1 convs keep the format, so the NHWC views below are no copies
                x = x.contiguous(memory_format=torch.channels_last)
            outs = []
            for i in range(13):
                y = self._block(i, x)
                self.block_taken.append("layers" if y is None else "fused")
                if y is None:
                    x = self.dw_bn[i](self._depthwise(i, x), *bn)
                    x = self.pw_bn[i](self._pointwise(i, x), *bn)
                else:
                    x = y
                if i + 1 in (5, 11, 13):
                    outs.append(_nhwc(x).to(dt))
        return outs

    def convs(self):
        return []

    def keras_layers(self):
        out = [("conv1", [("conv1/kernel:0", self.conv1.weight, "oihw")]), ("conv1_bn", _bn_weights("conv1_bn",
                                                                                                    self.conv1_bn))]
        for i in range(13):
            n = i + 1
            out.append(("conv_dw_%d" % n, [("conv_dw_%d/depthwise_kernel:0" % n, self.dw[i].weight, "dw")]))
            out.append(("conv_dw_%d_bn" % n, _bn_weights("conv_dw_%d_bn" % n, self.dw_bn[i])))
            out.append(("conv_pw_%d" % n, [("conv_pw_%d/kernel:0" % n, self.pw[i].weight, "oihw")]))
            out.append(("conv_pw_%d_bn" % n, _bn_weights("conv_pw_%d_bn" % n, self.pw_bn[i])))
        return out

    def feature_shapes(self, image_hw):
        return [(1, 1)] + self.feature_shapes_probe(image_hw)


class _DenseLayer(nn.Module):
    def __init__(self, cin, growth):
        super().__init__()
        self.bn1 = _BNAct(cin, "relu", eps=1.001e-5)
        self.conv1 = nn.Conv2d(cin, 4 * growth, 1, bias=False)
        self.bn2 = _BNAct(4 * growth, "relu", eps=1.001e-5)
        self.conv2 = nn.Conv2d(4 * growth, growth, 3, padding=1, bias=False)

    def forward(self, x):
        y = self.conv2(self.bn2(self.conv1(self.bn1(x))))
        return torch.cat([x, y], dim=1)


class DenseNet(nn.Module, _ShapeProbe):
    BLOCKS = {"densenet121": [6, 12, 24, 16], "densenet169": [6, 12, 32, 32], "densenet201": [6, 12, 48, 32]}

    def __init__(self, name: str = "densenet121", growth: int = 32):
        super().__init__()
        blocks = self.BLOCKS[name]
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 0, bias=False)
        self.conv1_bn = _BNAct(64, "relu", eps=1.001e-5)
        c = 64
        self.dense = nn.ModuleList()
        self.trans = nn.ModuleList()
        outs = []
        for i, n in enumerate(blocks):
            layers = nn.ModuleList()
            for _ in range(n):
                layers.append(_DenseLayer(c, growth))
                c += growth
            self.dense.append(layers)
            outs.append(c)
            if i != len(blocks) - 1:
                self.trans.append(nn.ModuleDict({"bn": _BNAct(c, "relu", eps=1.001e-5),
                                                 "conv": nn.Conv2d(c, c // 2, 1, bias=False)}))
                c = c // 2
        self.out_channels = outs

    def forward(self, x):
        dt = x.dtype
        with _autocast(x):
            x = _nchw(x)
            x = self.conv1_bn(self.conv1(F.pad(x, (3, 3, 3, 3))))
            x = F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2)
            outs = []
            for i, layers in enumerate(self.dense):
                for l in layers:
                    x = l(x)
                if i >= 1:
                    outs.append(_nhwc(x).to(dt))
                if i < len(self.trans):
                    t = self.trans[i]
                    x = F.avg_pool2d(t["conv"](t["bn"](x)), 2, 2)
        return outs

    def convs(self):
        return []

    def keras_layers(self):
        out = [("conv1/conv", [("conv1/conv/kernel:0", self.conv1.weight, "oihw")]),
               ("conv1/bn", _bn_weights("conv1/bn", self.conv1_bn))]
        for s, layers in enumerate(self.dense):
            for i, l in enumerate(layers):
                p = "conv{}_block{}".format(s + 2, i + 1)
                out += [(p + "_0_bn", _bn_weights(p + "_0_bn", l.bn1)),
                        (p + "_1_conv", [(p + "_1_conv/kernel:0", l.conv1.weight, "oihw")]),
                        (p + "_1_bn", _bn_weights(p + "_1_bn", l.bn2)),
                        (p + "_2_conv", [(p + "_2_conv/kernel:0", l.conv2.weight, "oihw")])]
            if s < len(self.trans):
                p = "pool{}".format(s + 2)
                t = self.trans[s]
                out += [(p + "_bn", _bn_weights(p + "_bn", t["bn"])),
                        (p + "_conv", [(p + "_conv/kernel:0", t["conv"].weight, "oihw")])]
        return out

    def feature_shapes(self, image_hw):
        return [(1, 1)] + self.feature_shapes_probe(image_hw)


def make_backbone(name: str) -> nn.Module:
    if name in VGG.CFG:
        return VGG(name)
    if name.startswith("mobilenet"):
        # keras-retinanet names: mobilenet{128,160,192,224}_{alpha}
        alpha = float(name.split("_")[1]) if "_" in name else 1.0
        return MobileNet(alpha)
    if name in DenseNet.BLOCKS:
        return DenseNet(name)
    raise ValueError("Backbone '{}' not recognized.".format(name))


from . import Backbone  # noqa: E402  (models/__init__ imports this module lazily)


class _GenericBackbone(Backbone):
    def validate(self):
        ok = self.backbone in self.allowed or any(self.backbone.startswith(a) for a in self.allowed if a.endswith("_"))
        if not ok:
            raise ValueError("Backbone ('{}') not in allowed backbones ({}).".format(self.backbone, self.allowed))

    def retinanet(self, num_classes, modifier=None, **kwargs):
        from .retinanet import RetinaNet
        model = RetinaNet(num_classes, backbone=self.backbone, **kwargs)
        if modifier is not None:
            model = modifier(model) or model
        return model

    def imagenet_filename(self):
        return "{}_weights_tf_dim_ordering_tf_kernels_notop.h5".format(self.backbone)


class VGGBackbone(_GenericBackbone):
    allowed = ("vgg16", "vgg19")


class MobileNetBackbone(_GenericBackbone):
    allowed = ("mobilenet128_", "mobilenet160_", "mobilenet192_", "mobilenet224_")


class DenseNetBackbone(_GenericBackbone):
    allowed = ("densenet121", "densenet169", "densenet201")


def lookup(name: str):
    if "vgg" in name:
        return VGGBackbone(name)
    if "mobilenet" in name:
        return MobileNetBackbone(name)
    if "densenet" in name:
        return DenseNetBackbone(name)
    raise NotImplementedError("Backbone class for  '{}' not implemented.".format(name))
