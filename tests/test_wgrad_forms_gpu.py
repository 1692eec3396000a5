"""Every weight-gradient candidate ``conv_wgrad.wgrad_candidates`` offers, in both forms the builder derives from one
description per kind: the plain form (a fresh fp32 gradient) and the accumulating form (into a gradient slot that
starts as a random fp32 base; the result is ``slot - base``), each against the fp32 PyTorch conv backward with the
bound of tests/test_winners_gpu.py (max |err| / max |ref| <= 1.5e-2: bf16 operands, fp32 accumulation).

The shapes are the smallest that offer every kind: ``w64`` and ``whalo`` (64 -> 64), the slab-free ``hip30`` /
``hip31`` (144 tiles, 273 pixels), a packed pyramid, and the narrow regression final with ``pad64`` / ``swap``.
(The kernels' own accumulate arithmetic at more shapes: tests/test_wgrad_direct_gpu.py, tests/test_wgrad_narrow_gpu.py;
the tuned winners at production shapes, plain and ``|s``: tests/test_winners_gpu.py.)"""
import pytest
import torch
import torch.nn.functional as F

from batchai_retinanet_horovod_coco_amd.ops import native_conv as NC

pytestmark = pytest.mark.gpu

TOL = 1.5e-2
HIP = ["hip%d" % v for v in list(range(16)) + list(range(20, 26))]
PYRAMID = [(13, 21), (7, 11), (4, 6)]
CASES = {
    # name: (N, levels, cin, cout, single-geometry?, names offered beside miopen)
    "c64": (1, [(9, 9)], 64, 64, True, HIP + ["w64", "whalo"]),
    "direct": (1, [(13, 21)], 256, 256, True, HIP + ["hip30", "hip31", "whalo"]),
    "pyramid": (2, PYRAMID, 256, 64, False, HIP + ["whalo"]),
    "narrow": (2, PYRAMID, 256, 36, False, HIP + ["pad64", "swap"]),
}
_DATA = {}


def _ref_wgrad(x, dy, shapes):
    """fp32 (cout, 3, 3, cin) weight gradient of the shared 3x3 / s1 / same conv over the packed levels."""
    N, cin, cout = x.shape[0], x.shape[-1], dy.shape[-1]
    dw, off = torch.zeros(cout, cin, 3, 3, device=x.device), 0
    for h, w in shapes:
        xl = x[:, off:off + h * w].reshape(N, h, w, cin).float().permute(0, 3, 1, 2)
        dl = dy[:, off:off + h * w].reshape(N, h, w, cout).float().permute(0, 3, 1, 2)
        with torch.enable_grad():
            wr = torch.zeros(cout, cin, 3, 3, device=x.device, requires_grad=True)
            dw += torch.autograd.grad(F.conv2d(xl, wr, padding=1), wr, dl)[0]
        off += h * w
    return dw.permute(0, 2, 3, 1).contiguous()


def _data(name, cuda):
    """Operands, geometry, builder arguments and the reference of a case: built once, shared, never modified."""
    if name in _DATA:
        return _DATA[name]
    N, shapes, cin, cout, single, names = CASES[name]
    gen = torch.Generator(device=cuda).manual_seed(11 + cout)
    P = sum(h * w for h, w in shapes)
    x = torch.randn(N, P, cin, device=cuda, generator=gen).clamp_min(0).bfloat16()
    dy = torch.randn(N, P, cout, device=cuda, generator=gen).bfloat16()
    w = torch.zeros(cout, 3, 3, cin, device=cuda, dtype=torch.bfloat16)
    ref = _ref_wgrad(x, dy, shapes)
    if single:
        (h, wd), = shapes
        x, dy = x.view(N, h, wd, cin), dy.view(N, h, wd, cout)
        scale = torch.rand(cout, device=cuda, generator=gen) + 0.5       # folded frozen-BN scale
        ref = ref * scale.view(-1, 1, 1, 1)
        g = NC.geom_single(N, h, wd, h, wd, 3, 1, (1, 1, 1, 1), cin, cout)
        kw = {"lib_fn": lambda: NC._miopen_wgrad(x, w, dy, 1, (1, 1, 1, 1), scale)}
    else:
        scale = None
        g = NC.geom_pyramid(N, shapes, cin, cout)
        kw = {"lib_fn": lambda: NC._miopen_pyramid_wgrad(x, w, dy, shapes),
              "extra": NC._narrow_wgrads(x, dy, shapes, cout)}
    base = torch.randn(cout, 3, 3, cin, device=cuda, generator=gen) * float(ref.abs().max())
    _DATA[name] = (x, dy, g, scale, kw, base, ref)
    return _DATA[name]


def _err(got, ref):
    return float((got.float() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_every_candidate_in_both_forms(cuda, name, monkeypatch):
    # (pad64 / swap dispatch their inner 64-wide weight gradient through the tuner: no race, its first candidate)
    monkeypatch.setenv("MXR_CONV_TUNE", "0")
    x, dy, g, scale, kw, base, ref = _data(name, cuda)
    plain = NC.wgrad_candidates(x, dy, g, scale, **kw)
    slot = base.clone()
    sink = NC.wgrad_candidates(x, dy, g, scale, sink=slot, **kw)
    assert sorted(plain) == sorted(sink) == sorted(CASES[name][5] + ["miopen"])
    worst = {}
    for n in plain:
        got = plain[n]()
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape), n
        slot.copy_(base)
        sink[n]()
        worst[n] = (_err(got, ref), _err(slot - base, ref))
    print(name, {n: "%.2e %.2e" % e for n, e in worst.items()})
    bad = {n: e for n, e in worst.items() if not max(e) <= TOL}
    assert not bad, bad
