"""The candidate names the forward / data-gradient dispatch offers (ops.conv_launch.FAMILIES and the per-pass
orders): the ordered lists recorded before the family table replaced the per-pass rule copies
(tests/fixtures/conv_candidates.json, written by scripts/record_conv_candidates.py), and the committed tuning
table's winners.  CPU: candidates are built, nothing is launched."""
import ast
import importlib.util
import json
import os

import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL
from batchai_retinanet_horovod_coco_amd.ops import fp8 as F8
from batchai_retinanet_horovod_coco_amd.ops import native_conv as NC

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
with open(os.path.join(ROOT, "tests", "fixtures", "conv_candidates.json")) as _f:
    RECORDED = json.load(_f)
with open(os.path.join(ROOT, "tuning", "conv_table.json")) as _f:
    # the bf16 keys of the two passes (fp8 keys / winners: the fp8 builders, tests/test_fp8_gpu.py)
    TABLE = {k: v for k, v in json.load(_f)["table"].items()
             if k.split("|")[0] in ("fwd", "dgrad") and "f8" not in k.split("|") and not v.startswith("f8")}


@pytest.fixture(scope="module")
def offered():
    spec = importlib.util.spec_from_file_location(
        "record_conv_candidates", os.path.join(ROOT, "scripts", "record_conv_candidates.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec.offered()


def test_every_recorded_list_is_rebuilt(offered):
    assert sorted(offered) == sorted(RECORDED) and len(RECORDED) > 150


@pytest.mark.parametrize("eid", sorted(RECORDED))
def test_offered_names_and_order_as_recorded(offered, eid):
    assert offered[eid] == RECORDED[eid]


def test_narrow_switch_and_fp8_are_recorded():
    """The recorded cases do exercise the switches (else the comparison above says nothing about them)."""
    narrow = "fwd|2,50,84,64,64,3,1,1111|plain"
    assert "hx32_8" in RECORDED[narrow] and "hx32_8" not in RECORDED[narrow + "|wide"]
    assert "hx32_8" in RECORDED["dgrad|2,50,84,64,64,3,1,1111|plain"]
    assert "hx32_8" not in RECORDED["dgrad|2,50,84,64,64,3,1,1111|plain|wide"]
    assert any(n.startswith("f8_") for n in RECORDED["fwd|2,50,84,256,256,3,1,1111|plain|f8"])
    assert any(n.startswith("f8d_") for n in RECORDED["dgrad|2,50,84,256,256,3,1,1111|plain|f8"])


def _table_names(key):
    """Names offered for a committed ``fwd|`` / ``dgrad|`` key, after the BitMask filter of ``|eb`` / ``|mb``."""
    p = key.split("|")
    N, H, W, cin, cout, k, stride = (int(v) for v in p[1:8])
    pads = ast.literal_eval(p[8])
    Ho, Wo = NC._out_hw(H, W, k, stride, pads)
    x = torch.zeros(N, H, W, cin, dtype=torch.bfloat16, device="meta")
    w = torch.zeros(cout, k, k, cin, dtype=torch.bfloat16, device="meta")
    if p[0] == "fwd":
        relu, res, flags = int(p[9]), int(p[10]), p[11:]
        g = NC.geom_single(N, H, W, Ho, Wo, k, stride, pads, cin, cout)
        r = torch.zeros(N, Ho, Wo, cout, dtype=torch.bfloat16, device="meta") if res else None
        names = list(NC.fwd_candidates(x, w, None, r, g, stride, pads, bool(relu), (N, Ho, Wo, cout), fp8_ok=True))
    else:
        flags = p[9:]
        dy = torch.zeros(N, Ho, Wo, cout, dtype=torch.bfloat16, device="meta")
        kw = {"mask": x} if ("m" in flags or "mb" in flags) else {}
        if "a" in flags:
            kw["out"] = torch.zeros_like(x)
        names = list(NC._dgrad_cands(dy, w, x, stride, pads, **kw))
    if "eb" in flags or "mb" in flags:
        names = [n for n in names if NC.bits_capable(n)]
    return names


def test_table_has_keys_of_both_passes():
    assert {k.split("|")[0] for k in TABLE} == {"fwd", "dgrad"}


@pytest.mark.parametrize("key", sorted(TABLE))
def test_committed_winner_is_offered(key):
    assert not F8.enabled()
    assert TABLE[key] in _table_names(key), key


def test_family_lookup():
    assert CL.family_of("hx32_11").prefix == "hx32_" and CL.family_of("c1p").prefix == "c1p"
    assert CL.family_of("hip14").prefix == "hip" and CL.family_of("halo0").prefix == "halo"
    assert CL.family_of("c1x1_65").prefix == "c1x1_" and CL.family_of("p8_5").prefix == "p8_"
    assert CL.family_of("sk11").prefix == "sk"
    for name in ("miopen", "f8_0", "f8d_10", "nope", "", "h", "hx32", "c1x1"):
        assert CL.family_of(name) is None and not CL.bits_capable(name), name
    assert set(CL.FWD_ORDER) == {f.prefix for f in CL.FAMILIES}
