"""``sepblock_stream.hip`` (``mxr_sepblock_stream_fwd``) against float64 on the CPU, by the method, the oracle and the
allowance of ``tests/test_sepblock_gpu.py``: ``2^-8 (|y_ref| + |a2| sum_ci |w2| z_ref) + 1e-5`` per element, no element
excluded; the oracle itself asserts that both clamps are hit in ``Z`` and ``y`` and that a third of ``y`` lies inside
(0, 6).  Each case prints its worst error / allowance (``pytest -s``; profiles/sepblock_stream_gpu_tests.log).
"""
import pytest
import torch
import torch.nn as nn

from batchai_retinanet_horovod_coco_amd.models.extra_backbones import MobileNet
from batchai_retinanet_horovod_coco_amd.ops import native as N
from batchai_retinanet_horovod_coco_amd.ops import separable as SB
from test_sepblock_gpu import case, operands

pytestmark = pytest.mark.gpu

# (264, 256): 9 chunks (odd: ring parity), an 8-channel last chunk, half the waves idle; (512, 520): a full column block
# and a second one of 8 channels; (288, 1024): two full column blocks
RULE_CASES = [(ci, co, s, nhw) for ci, co in ((264, 256), (512, 520), (288, 1024)) for s in (1, 2)
              for nhw in ((1, 1, 1), (2, 5, 7), (3, 9, 35)) if s == 1 or nhw != (1, 1, 1)]
# shapes the rule leaves to the resident kernel: the smallest Ci, a Co that is no multiple of 64
NAMED_CASES = [(ci, co, s, (2, 9, 35)) for ci, co in ((32, 8), (160, 136)) for s in (1, 2)]


def check(out, again, ci, co, stride, nhw):
    ref, allow = case(ci, co, stride, nhw)[5:]
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    assert torch.equal(out, again), "repeat calls differ"
    err = (out.cpu().double() - ref).abs()
    print("\nstream: Ci {} Co {} stride {} NHW {}: worst |err| / allowance {:.3f}".format(
        ci, co, stride, nhw, float((err / allow).max())))
    assert bool((err <= allow).all())


@pytest.mark.parametrize("ci,co,stride,nhw", RULE_CASES)
def test_rule_takes_stream_against_float64(cuda, ci, co, stride, nhw):
    assert N.sepblock_form(ci, co) == "stream"
    ops = operands(ci, co, stride, nhw, cuda)
    with torch.no_grad():
        out = SB.separable_block_eval(*ops, backend="native")
        again = SB.separable_block_eval(*ops, backend="native")
    check(out, again, ci, co, stride, nhw)


def named(ops, form):
    x, wdw, bn1, wpw, bn2, stride = ops
    return N.sepblock_fwd(x, N.dwconv_taps(wdw), SB._bn_operands(bn1), N.pwconv_weight(wpw), SB._bn_operands(bn2),
                          stride, form=form)


@pytest.mark.parametrize("ci,co,stride,nhw", NAMED_CASES)
def test_named_stream_against_float64(cuda, ci, co, stride, nhw):
    assert N.sepblock_form(ci, co) == "resident"
    ops = operands(ci, co, stride, nhw, cuda)
    check(named(ops, "stream"), named(ops, "stream"), ci, co, stride, nhw)


def test_named_stream_refuses_ci24(cuda):
    ops = operands(24, 40, 1, (2, 5, 7), cuda)
    assert named(ops, "resident").shape == (2, 5, 7, 40)
    with pytest.raises(N.NotServed):
        named(ops, "stream")


def test_captured_stream_call_replays_bit_equal(cuda):
    ci, co, stride, nhw = 264, 256, 2, (2, 9, 35)
    ops = operands(ci, co, stride, nhw, cuda)
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(*nhw, ci, generator=g).bfloat16().to(cuda) for _ in range(3)]
    with torch.no_grad():
        SB.separable_block_eval(*ops, backend="native")          # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = SB.separable_block_eval(*ops, backend="native")
        for new in xs + xs:                                      # several replays on new input
            ops[0].copy_(new)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, SB.separable_block_eval(*ops, backend="native"))
    torch.cuda.synchronize()                                     # no replay in flight when the graph and its pool go


def test_mobilenet_wide_blocks_fused_against_float64(cuda):
    """C3..C5 of MobileNet(1.0).eval(), bf16, 2 x 64 x 96, statistics as in test_mobilenet_fused_against_float64: blocks
    7 to 13 take the stream form.  The fused path rounds less than the per-layer native path, so its max-abs deviation
    from the float64 CPU model should not be the larger one; 1.25x is allowed for layer-to-layer noise."""
    torch.manual_seed(5)
    ref = MobileNet(1.0).double()
    x = torch.randn(2, 64, 96, 3).bfloat16()
    bns = [m for m in ref.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        for m in bns:
            m.momentum = 1.0
        ref(x.double())                                          # running statistics = this batch's
        for m in bns:
            m.running_var.mul_(torch.rand(m.num_features).double() * 1.5 + 0.5)
            m.running_mean.add_(torch.randn(m.num_features).double() * 0.1 * m.running_var.sqrt())
        want = ref.eval()(x.double())
        dev = {}
        for arm in ("layers", "fused"):
            m = MobileNet(1.0)
            m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
            m.dw_backend = m.bn_backend = m.pw_backend = "native"
            m.block_backend = "native" if arm == "fused" else "torch"
            got = m.to(cuda).eval()(x.to(cuda))
            assert m.block_taken == [arm] * 13
            dev[arm] = [float((a.double().cpu() - r).abs().max()) for a, r in zip(got, want)]
    forms = [N.sepblock_form(ci, co) for ci, co in zip([32] + MobileNet.FILTERS[:-1], MobileNet.FILTERS)]
    assert forms == ["resident"] * 6 + ["stream"] * 7
    for name, r, lay, fus in zip(("C3", "C4", "C5"), want, dev["layers"], dev["fused"]):
        print("\nMobileNet(1.0) {}: per-layer native {:.4e}, fused {:.4e}, ratio {:.3f} (max |ref| {:.3f})".format(
            name, lay, fus, fus / lay, float(r.abs().max())))
    for name, lay, fus in zip(("C3", "C4", "C5"), dev["layers"], dev["fused"]):
        assert fus <= 1.25 * lay, name
