"""The candidate names the weight-gradient builder offers (ops.conv_wgrad.wgrad_candidates), per shape and form, in
race order, and what each ``only=`` single-candidate build yields.  tests/fixtures/wgrad_candidates.json was written
from the commit before that one builder replaced ``wgrad_candidates`` / ``_only_wgrad`` / ``_wgrad_sink_cands`` and
the pyramid layer's ``sink_make`` closure, by a throwaway variant of scripts/record_wgrad_candidates.py whose
``names()`` called those builders as their callers composed them (``miopen`` appended to the plain sets, ``pad64`` /
``swap`` after it).  CPU: candidates are built, nothing is launched."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
with open(os.path.join(ROOT, "tests", "fixtures", "wgrad_candidates.json")) as _f:
    RECORDED = json.load(_f)
HIP = ["hip%d" % v for v in list(range(16)) + list(range(20, 26))]


@pytest.fixture(scope="module")
def offered():
    spec = importlib.util.spec_from_file_location(
        "record_wgrad_candidates", os.path.join(ROOT, "scripts", "record_wgrad_candidates.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec.offered()


def test_every_recorded_list_is_rebuilt(offered):
    # 17 single shapes and 4 pyramid widths in 3 forms, the narrow final in 2 x 2 more; each with its only= builds
    assert sorted(offered) == sorted(RECORDED) and len(RECORDED) == 2 * (21 * 3 + 4)


@pytest.mark.parametrize("eid", sorted(RECORDED))
def test_offered_names_and_order_as_recorded(offered, eid):
    assert offered[eid] == RECORDED[eid]


def test_only_builds_exactly_the_offered_name():
    for eid, names in RECORDED.items():
        if not eid.endswith("|only"):
            only = RECORDED[eid + "|only"]
            assert set(names) <= set(only) and "nope" in only
            for n, built in only.items():
                assert built == ([n] if n in names else []), (eid, n)


def test_recorded_anchors():
    """The orders of the two forms differ in where ``miopen`` sits; both are part of the tuning (first listed wins
    under capture and with tuning off, ties keep the earlier name)."""
    r = RECORDED
    assert r["wgrad|2,50,84,64,64,3,1|plain"] == HIP + ["w64", "whalo"]
    assert r["wgrad|2,50,84,64,64,3,1|plain+lib"] == HIP + ["w64", "whalo", "miopen"]
    assert r["wgrad|2,50,84,64,64,3,1|sink"] == HIP + ["miopen", "w64", "whalo"]
    assert r["wgrad|1,13,21,256,256,3,1|plain"] == HIP + ["hip30", "hip31", "whalo"]
    assert r["wgrad|1,13,21,256,256,3,1|sink"] == HIP + ["hip30", "hip31", "miopen", "whalo"]
    assert r["pwgrad|64|plain"] == HIP + ["whalo"]
    assert r["pwgrad|64|sink"] == HIP + ["miopen", "whalo"]
    assert r["pwgrad|36|plain+narrow|swap"] == HIP + ["miopen", "pad64", "swap"]
    assert r["pwgrad|36|sink+narrow|swap"] == HIP + ["miopen", "pad64", "swap"]
    assert r["pwgrad|36|plain+narrow|noswap"] == r["pwgrad|36|sink+narrow|noswap"] == HIP + ["miopen", "pad64"]
