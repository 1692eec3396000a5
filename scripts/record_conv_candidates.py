"""Candidate names the forward / data-gradient dispatch offers, per shape and form, in race order (CPU only:
candidates are built, nothing is launched).

    python scripts/record_conv_candidates.py > tests/fixtures/conv_candidates.json

tests/test_conv_candidates.py compares :func:`offered` with the committed file, which was written from the
commit before the kernel-family table (ops.conv_launch.FAMILIES) replaced the per-pass rule copies."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from batchai_retinanet_horovod_coco_amd.ops import conv_launch as CL  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import fp8 as F8  # noqa: E402
from batchai_retinanet_horovod_coco_amd.ops import native_conv as NC  # noqa: E402

SINGLE = [
    # N, H, W, cin, cout, k, stride, pads
    (2, 50, 84, 256, 256, 3, 1, (1, 1, 1, 1)),
    (2, 50, 84, 1024, 256, 1, 1, (0, 0, 0, 0)),
    (2, 50, 84, 256, 1024, 1, 1, (0, 0, 0, 0)),
    (2, 50, 84, 64, 64, 3, 1, (1, 1, 1, 1)),
    (2, 100, 167, 64, 256, 1, 1, (0, 0, 0, 0)),
    (2, 25, 42, 512, 512, 3, 2, (1, 1, 1, 1)),
    (2, 50, 84, 256, 512, 1, 2, (0, 0, 0, 0)),
    (1, 13, 21, 256, 256, 3, 2, (1, 1, 1, 1)),
    (2, 7, 11, 2048, 256, 1, 1, (0, 0, 0, 0)),
    (2, 50, 84, 128, 128, 3, 1, (1, 1, 1, 1)),
    (2, 200, 334, 64, 64, 1, 1, (0, 0, 0, 0)),
    (2, 100, 167, 256, 64, 1, 1, (0, 0, 0, 0)),
    (2, 100, 167, 256, 128, 1, 1, (0, 0, 0, 0)),
    (1, 9, 9, 64, 36, 3, 1, (1, 1, 1, 1)),
    (1, 9, 9, 96, 72, 1, 1, (0, 0, 0, 0)),
    (1, 9, 9, 64, 12, 1, 1, (0, 0, 0, 0)),
]
NARROW_OFF = SINGLE[3]      # the 64-channel 3x3 layer, also recorded with NARROW_TILES off
PYRAMID = ([(13, 21), (7, 11), (4, 6)], 256, (256, 720, 64, 36))
FWD_FORMS = ("plain", "out")
DGRAD_FORMS = ("plain", "mask", "out", "res")


def single(case, form, dgrad):
    """Ordered names of one single-level case: forward, or its data gradient."""
    N, H, W, cin, cout, k, stride, pads = case
    Ho, Wo = NC._out_hw(H, W, k, stride, pads)
    x = torch.zeros(N, H, W, cin, dtype=torch.bfloat16)
    w = torch.zeros(cout, k, k, cin, dtype=torch.bfloat16)
    if not dgrad:
        g = NC.geom_single(N, H, W, Ho, Wo, k, stride, pads, cin, cout)
        out = torch.zeros(N, Ho, Wo, cout, dtype=torch.bfloat16) if form == "out" else None
        return list(NC.fwd_candidates(x, w, None, None, g, stride, pads, True, (N, Ho, Wo, cout), fp8_ok=True, out=out))
    dy = torch.zeros(N, Ho, Wo, cout, dtype=torch.bfloat16)
    kw = {"mask": {"mask": x}, "out": {"out": torch.zeros_like(x)}, "res": {"res": x}}.get(form, {})
    return list(NC._dgrad_cands(dy, w, x, stride, pads, **kw))


def pyramid(cout, form):
    shapes, cin, _ = PYRAMID
    g = NC.geom_pyramid(2, shapes, cin, cout)
    P = int(g.M) // 2
    x = torch.zeros(2, P, cin, dtype=torch.bfloat16)
    w = torch.zeros(cout, 3, 3, cin, dtype=torch.bfloat16)
    out = torch.zeros(2, P, cout, dtype=torch.bfloat16) if form == "out" else None
    return list(NC.fwd_candidates(x, w, None, None, g, 1, (1, 1, 1, 1), True, (2, P, cout), allow_miopen=False,
                                  fp8_ok=True, out=out))


def entries():
    """(id, thunk) of every recorded list; the id says which switches the thunk runs under."""
    for fp8 in (False, True):
        tag = "|f8" if fp8 else ""
        for case in SINGLE:
            cid = ",".join(str(v) for v in case[:7]) + "," + "".join(str(p) for p in case[7])
            for form in FWD_FORMS:
                yield "fwd|%s|%s%s" % (cid, form, tag), fp8, True, (lambda c=case, f=form: single(c, f, False))
            for form in DGRAD_FORMS:
                if form != "res" or case[6] == 1:
                    yield "dgrad|%s|%s%s" % (cid, form, tag), fp8, True, (lambda c=case, f=form: single(c, f, True))
            if case is NARROW_OFF and not fp8:
                yield "fwd|%s|plain|wide" % cid, fp8, False, (lambda c=case: single(c, "plain", False))
                yield "dgrad|%s|plain|wide" % cid, fp8, False, (lambda c=case: single(c, "plain", True))
        for cout in PYRAMID[2]:
            for form in FWD_FORMS:
                yield "pfwd|%d|%s%s" % (cout, form, tag), fp8, True, (lambda c=cout, f=form: pyramid(c, f))


def offered():
    """{id: ordered names} plus, under "bits_capable", the BitMask flag of every name seen."""
    rec, names = {}, set()
    was, narrow = F8.enabled(), CL.NARROW_TILES
    try:
        for eid, fp8, nar, thunk in entries():
            F8.set_enabled(fp8)
            CL.NARROW_TILES = nar
            rec[eid] = thunk()
            names.update(rec[eid])
    finally:
        F8.set_enabled(was)
        CL.NARROW_TILES = narrow
    rec["bits_capable"] = {n: bool(NC.bits_capable(n)) for n in sorted(names)}
    return rec


if __name__ == "__main__":
    rec = offered()      # one entry per line
    sys.stdout.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rec[k], sort_keys=True))
                                        for k in sorted(rec)) + "\n}\n")
