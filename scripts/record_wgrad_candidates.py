"""Candidate names the weight-gradient dispatch offers (ops.conv_wgrad.wgrad_candidates), per shape and form, in
race order, and what every ``only=`` single-candidate build of each list yields (CPU only: candidates are built,
nothing is launched).

    python scripts/record_wgrad_candidates.py > tests/fixtures/wgrad_candidates.json

tests/test_wgrad_candidates.py compares :func:`offered` with the committed file.  The shapes are those of
scripts/record_conv_candidates.py and :data:`DIRECT`.  Forms: ``plain`` (fresh tensor, no library form),
``plain+lib`` (what ``run_wgrad`` races without a gradient sink), ``sink`` (accumulating into the parameter's slot)
and, for the narrow regression final, ``plain+narrow`` / ``sink+narrow`` (the pyramid layer's sets with ``pad64`` /
``swap``) with ``native_conv.SWAP_NARROW_WGRAD`` on and off."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
from batchai_retinanet_horovod_coco_amd.ops import conv_wgrad as CW  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native_conv as NC  # noqa: E402
from record_conv_candidates import PYRAMID, SINGLE  # noqa: E402

FORMS = ("plain", "plain+lib", "sink")
NARROW_FORMS = ("plain+narrow", "sink+narrow")
DIRECT = (1, 13, 21, 256, 256, 3, 1, (1, 1, 1, 1))     # a shape the slab-free forms (hip30 / hip31) and whalo cover
PROBES = ("nope", "hip2", "hip30", "hip99", "w64", "whalo", "miopen", "pad64", "swap")   # only= names, offered or not


def _lib():
    return None


def names(x, dy, g, form, only=None, extra=None):
    """Ordered names of one build of the candidate set."""
    sink = torch.zeros(g.cout * g.kh * g.kw * g.cin) if form.startswith("sink") else None
    return list(CW.wgrad_candidates(x, dy, g, None, only=only, sink=sink, lib_fn=None if form == "plain" else _lib,
                                    extra=extra))


def narrow(x, dy, shapes, cout):
    """The pyramid layer's extra forms for a narrow final (None for the others)."""
    return NC._narrow_wgrads(x, dy, shapes, cout)


def _single(case):
    N, H, W, cin, cout, k, stride, pads = case
    Ho, Wo = NC._out_hw(H, W, k, stride, pads)
    x = torch.zeros(N, H, W, cin, dtype=torch.bfloat16)
    dy = torch.zeros(N, Ho, Wo, cout, dtype=torch.bfloat16)
    return x, dy, NC.geom_single(N, H, W, Ho, Wo, k, stride, pads, cin, cout)


def _pyramid(cout):
    shapes, cin, _ = PYRAMID
    g = NC.geom_pyramid(2, shapes, cin, cout)
    P = int(g.M) // 2
    return torch.zeros(2, P, cin, dtype=torch.bfloat16), torch.zeros(2, P, cout, dtype=torch.bfloat16), g


def entries():
    """(id, x, dy, g, form, swap switch or None) of every recorded list."""
    for case in SINGLE + [DIRECT]:
        cid = ",".join(str(v) for v in case[:7])
        for form in FORMS:
            yield ("wgrad|%s|%s" % (cid, form),) + _single(case) + (form, None)
    for cout in PYRAMID[2]:
        for form in FORMS:
            yield ("pwgrad|%d|%s" % (cout, form),) + _pyramid(cout) + (form, None)
        if cout % 8 and cout < 64:
            for form in NARROW_FORMS:
                for swap in (True, False):
                    eid = "pwgrad|%d|%s|%s" % (cout, form, "swap" if swap else "noswap")
                    yield (eid,) + _pyramid(cout) + (form, swap)


def offered():
    """{id: ordered names, id + "|only": {name: names of the only=name build}} for every offered name and each
    of :data:`PROBES`."""
    rec = {}
    was = NC.SWAP_NARROW_WGRAD
    try:
        for eid, x, dy, g, form, swap in entries():
            extra = None
            if swap is not None:
                NC.SWAP_NARROW_WGRAD = swap
                extra = narrow(x, dy, PYRAMID[0], g.cout)
            rec[eid] = names(x, dy, g, form, extra=extra)
            probes = rec[eid] + [n for n in PROBES if n not in rec[eid]]
            rec[eid + "|only"] = {n: names(x, dy, g, form, only=n, extra=extra) for n in probes}
    finally:
        NC.SWAP_NARROW_WGRAD = was
    return rec


if __name__ == "__main__":
    rec = offered()      # one entry per line
    sys.stdout.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rec[k], sort_keys=True))
                                        for k in sorted(rec)) + "\n}\n")
