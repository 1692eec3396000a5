"""CPU: the ordered host-side events of every weight / bias gradient delivery (ops.conv_wgrad, ops.fp8): which
candidates are built and handed to the tuner under which key, what each launch writes to (the parameter's slot in
the flat gradient buffer, or a scratch clone of it while the tuner races), whether it runs inside a side-stream
region and what that region reads, and that every parameter is notified after its launch and inside the region.

The sinks, the side stream, the tuner and the launchers are fakes that append to one event list.  The lists were
written against the commit before the five delivery copies became ``conv_wgrad._deliver`` (there with the pyramid
layer's call spelled through its ``_deliver_wgrad`` and ``sink_make`` closure) and passed there unchanged."""
import pytest
import torch

from batchai_retinanet_horovod_coco_amd.ops import conv_tuner as CT
from batchai_retinanet_horovod_coco_amd.ops import conv_wgrad as CW
from batchai_retinanet_horovod_coco_amd.ops import fp8 as F8
from batchai_retinanet_horovod_coco_amd.ops import native_conv as NC
from batchai_retinanet_horovod_coco_amd.ops import side_stream as SS

HIP = ["hip%d" % v for v in list(range(16)) + list(range(20, 26))]


class _Param:
    def __init__(self, name, main=False):
        self.name = name
        if main:
            self.mxr_main_wgrad = True


class _Sinks:
    def __init__(self, ev, slots):
        self.ev, self.slots = ev, slots

    def get(self, p):
        return self.slots.get(p)

    def notify(self, p):
        self.ev.append(("notify", p.name))


class _Region:
    def __init__(self, h, reads):
        self.h, self.reads = h, reads

    def __enter__(self):
        self.h.ev.append(("enter",) + tuple(self.h.label(t) for t in self.reads))
        return self

    def __exit__(self, *exc):
        self.h.ev.append(("exit",))
        return False


class _Side:
    def __init__(self, h, usable):
        self.h, self.answer = h, usable

    def usable(self, t):
        self.h.ev.append(("usable", self.h.label(t), self.answer))
        return self.answer

    def run(self, device, *reads):
        assert isinstance(device, torch.device)
        return _Region(self.h, reads)


class _Tuner:
    """Runs the table's winner when it is among the candidates, else the first one (no timing)."""
    key = staticmethod(CT.ConvTuner.key)

    def __init__(self, h, table, tune, prefer):
        self.h, self.table, self.tune, self.prefer_answer = h, dict(table), tune, prefer
        self.calls, self.timings, self.borrowed = {}, {}, {}

    def winner(self, key):
        return self.table.get(key)

    def needs_tuning(self, key, names):
        self.h.ev.append(("needs_tuning", key, list(names)))
        return self.tune

    def prefer(self, key, name, margin_ms):
        self.h.ev.append(("prefer", key, name, margin_ms))
        if self.prefer_answer:
            self.table[key] = name
        return self.prefer_answer

    def run(self, key, cands):
        self.calls[key] = self.calls.get(key, 0) + 1
        self.h.ev.append(("tuner.run", key, list(cands)))
        name = self.table.get(key)
        return cands[name if name in cands else next(iter(cands))]()


class _DualLib:
    def __init__(self, h):
        self.h = h

    def mxr_conv_wgrad_p8_dual(self, *a):
        self.h.ev.append(("dual", a[14], self.h.where(a[7]), self.h.where(a[8])))
        return 0


class Harness:
    """One event list; tensors are named by :meth:`name`, gradient slots by :meth:`slot`."""

    def __init__(self, monkeypatch, usable=False, table=(), tune=False, prefer=False):
        self.ev, self.names, self.slots, self.ptrs = [], {}, {}, {}
        self.result = torch.zeros(1)
        self.tuner = _Tuner(self, dict(table), tune, prefer)
        side = _Side(self, usable)
        monkeypatch.setattr(CT, "TUNER", self.tuner)
        monkeypatch.setattr(CW, "SIDE", side)
        monkeypatch.setattr(SS, "SIDE", side)
        monkeypatch.setattr(CW._n, "grad_sinks", lambda: _Sinks(self.ev, self.slots))
        monkeypatch.setattr(CW, "conv_wgrad", self._conv_wgrad)
        monkeypatch.setattr(CW, "halo_wgrad", self._halo_wgrad)
        monkeypatch.setattr(CW, "bias_grad", self._bias_grad)
        monkeypatch.setattr(F8, "pyramid_wgrad", self._f8_wgrad)
        monkeypatch.setattr(CW, "lib", lambda: _DualLib(self))
        monkeypatch.setattr(CW, "_s", lambda: 0)
        monkeypatch.setenv("MXR_WGRAD_FUSED_BIAS", "1")

    def name(self, label, t):
        self.names[id(t)] = label
        return t

    def slot(self, param, shape):
        t = self.name(param.name + ".slot", torch.zeros(shape))
        self.slots[param] = t
        self.ptrs[t.data_ptr()] = param.name + ".slot"
        return t

    def label(self, t):
        return None if t is None else self.names.get(id(t), "?")

    def where(self, out):
        """A launch's output: None, a parameter's slot (or a view of it), or a scratch clone."""
        if out is None:
            return None
        ptr = out if isinstance(out, int) else out.data_ptr()
        return self.ptrs.get(ptr, "clone")

    def _conv_wgrad(self, x, dy, g, scale, out=None, accumulate=False, variant=None, bias_out=None,
                    bias_accumulate=False):
        e = ("conv_wgrad", self.label(x), self.label(dy), self.label(scale), variant, self.where(out), accumulate)
        self.ev.append(e + ((self.where(bias_out), bias_accumulate) if bias_out is not None else ()))
        return self.result if out is None else out

    def _halo_wgrad(self, x, dy, g, scale=None, out=None, accumulate=False):
        self.ev.append(("halo_wgrad", self.where(out), None if out is None else tuple(out.shape), accumulate))
        return self.result if out is None else out

    def _bias_grad(self, dy, scale=None, out=None, accumulate=False, channels=None):
        self.ev.append(("bias_grad", self.label(dy), self.label(scale), self.where(out), accumulate, channels))
        return self.result if out is None else out

    def _f8_wgrad(self, xq, ix, dq, idq, g, out=None, accumulate=False, variant=0, splits=None, bias_out=None,
                  bias_accumulate=False):
        self.ev.append(("f8_wgrad", self.where(out), None if out is None else tuple(out.shape), accumulate, variant,
                        self.where(bias_out), bias_accumulate))
        return self.result if out is None else out


# ---------------------------------------------------------------- weight gradient: run_wgrad
def _single(h, main=False, sink=True):
    x = h.name("x", torch.zeros(1, 9, 9, 64, dtype=torch.bfloat16))
    dy = h.name("dy", torch.zeros(1, 9, 9, 64, dtype=torch.bfloat16))
    scale = h.name("scale", torch.ones(64))
    w = torch.zeros(64, 3, 3, 64)
    p = _Param("w", main)
    if sink:
        h.slot(p, tuple(w.shape))
    return x, dy, w, scale, p


KEY = "wgrad|1|9|9|64|64|3|1|(1, 1, 1, 1)"
PLAIN = HIP + ["w64", "whalo", "miopen"]
SINK = HIP + ["miopen", "w64", "whalo"]


def _launch(variant, where):
    return ("conv_wgrad", "x", "dy", "scale", variant, where, where is not None)


def test_wgrad_without_a_sink_races_the_plain_set(monkeypatch):
    h = Harness(monkeypatch, usable=True)
    x, dy, w, scale, p = _single(h, sink=False)
    assert CW.run_wgrad(x, dy, w, 1, (1, 1, 1, 1), scale, p) is h.result
    assert h.ev == [("tuner.run", KEY, PLAIN), _launch(0, None)]


def test_wgrad_winner_builds_one_candidate(monkeypatch):
    h = Harness(monkeypatch, table={KEY + "|s": "hip23"})
    x, dy, w, scale, p = _single(h)
    assert CW.run_wgrad(x, dy, w, 1, (1, 1, 1, 1), scale, p) is None
    assert h.ev == [("usable", "w.slot", False), ("tuner.run", KEY + "|s", ["hip23"]), _launch(23, "w.slot"),
                    ("notify", "w")]


def test_wgrad_winner_sees_the_slot_in_the_kernel_shape(monkeypatch):
    h = Harness(monkeypatch, table={KEY + "|s": "whalo"})
    x, dy, w, scale, p = _single(h)
    assert CW.run_wgrad(x, dy, w, 1, (1, 1, 1, 1), scale, p) is None
    assert h.ev == [("usable", "w.slot", False), ("tuner.run", KEY + "|s", ["whalo"]),
                    ("halo_wgrad", "w.slot", (64, 3, 3, 64), True), ("notify", "w")]


@pytest.mark.parametrize("winner", ["swap", None])
def test_wgrad_without_a_usable_winner_builds_the_full_set(monkeypatch, winner):
    h = Harness(monkeypatch, table={KEY + "|s": winner} if winner else {})
    x, dy, w, scale, p = _single(h)
    assert CW.run_wgrad(x, dy, w, 1, (1, 1, 1, 1), scale, p) is None
    assert h.ev == [("needs_tuning", KEY + "|s", SINK), ("usable", "w.slot", False),
                    ("tuner.run", KEY + "|s", SINK), _launch(0, "w.slot"), ("notify", "w")]


def test_wgrad_first_sight_races_on_a_clone_then_runs_serially(monkeypatch):
    h = Harness(monkeypatch, usable=True, tune=True)
    x, dy, w, scale, p = _single(h)
    assert CW.run_wgrad(x, dy, w, 1, (1, 1, 1, 1), scale, p) is None
    assert h.ev == [("needs_tuning", KEY + "|s", SINK),
                    ("tuner.run", KEY + "|s", SINK), _launch(0, "clone"),
                    ("tuner.run", KEY + "|s", SINK), _launch(0, "w.slot"), ("notify", "w")]
    assert h.tuner.calls == {KEY + "|s": 2}


def test_wgrad_on_the_side_stream(monkeypatch):
    h = Harness(monkeypatch, usable=True, table={KEY + "|s": "hip23"})
    x, dy, w, scale, p = _single(h)
    assert CW.run_wgrad(x, dy, w, 1, (1, 1, 1, 1), scale, p) is None
    assert h.ev == [("usable", "w.slot", True), ("enter", "x", "dy", "scale"),
                    ("tuner.run", KEY + "|s", ["hip23"]), _launch(23, "w.slot"), ("notify", "w"), ("exit",)]


def test_wgrad_of_a_main_stream_parameter_is_serial(monkeypatch):
    h = Harness(monkeypatch, usable=True, table={KEY + "|s": "hip23"})
    x, dy, w, scale, p = _single(h, main=True)
    assert CW.run_wgrad(x, dy, w, 1, (1, 1, 1, 1), scale, p) is None
    assert h.ev == [("usable", "w.slot", True), ("tuner.run", KEY + "|s", ["hip23"]), _launch(23, "w.slot"),
                    ("notify", "w")]


# ---------------------------------------------------------------- weight gradient: the pyramid layer's call
SHAPES = [(4, 6), (2, 3)]
PKEY = "pwgrad|2|((4, 6), (2, 3))|64|36"


def _pyramid(h, monkeypatch, sink=True):
    g = NC.geom_pyramid(2, SHAPES, 64, 36)
    P = int(g.M) // 2
    x = h.name("x", torch.zeros(2, P, 64, dtype=torch.bfloat16))
    dy = h.name("dy", torch.zeros(2, P, 64, dtype=torch.bfloat16))
    p = _Param("w")
    if sink:
        h.slot(p, (36, 3, 3, 64))
    narrow = []
    monkeypatch.setattr(NC, "_pad64_pwgrad", lambda *a: narrow.append("pad64") or torch.ones(36, 3, 3, 64))
    monkeypatch.setattr(NC, "_swap_pwgrad", lambda *a: narrow.append("swap") or torch.ones(36, 3, 3, 64))
    return x, dy, g, p, narrow


def _pyramid_wgrad(x, dy, g, p):
    """``PyramidConvFn.backward``'s weight-gradient call for the narrow regression final."""
    return CW.deliver_wgrad(PKEY, x, dy, g, None, p, (x, dy), lambda: torch.zeros(36, 3, 3, 64),
                            extra=NC._narrow_wgrads(x, dy, SHAPES, 36))


def _plaunch(variant, where):
    return ("conv_wgrad", "x", "dy", None, variant, where, where is not None)


def test_pyramid_wgrad_sets(monkeypatch):
    h = Harness(monkeypatch, usable=True)
    x, dy, g, p, narrow = _pyramid(h, monkeypatch, sink=False)
    assert _pyramid_wgrad(x, dy, g, p) is h.result
    assert h.ev == [("tuner.run", PKEY, HIP + ["miopen", "pad64", "swap"]), _plaunch(0, None)]
    h = Harness(monkeypatch, usable=True)
    x, dy, g, p, narrow = _pyramid(h, monkeypatch)
    assert _pyramid_wgrad(x, dy, g, p) is None
    assert h.ev == [("needs_tuning", PKEY + "|s", HIP + ["miopen", "pad64", "swap"]), ("usable", "w.slot", True),
                    ("enter", "x", "dy"), ("tuner.run", PKEY + "|s", HIP + ["miopen", "pad64", "swap"]),
                    _plaunch(0, "w.slot"), ("notify", "w"), ("exit",)]


@pytest.mark.parametrize("winner", ["pad64", "swap", "miopen"])
def test_pyramid_wgrad_fresh_tensor_forms_are_added_to_the_slot(monkeypatch, winner):
    h = Harness(monkeypatch, usable=True, table={PKEY + "|s": winner})
    x, dy, g, p, narrow = _pyramid(h, monkeypatch)
    assert _pyramid_wgrad(x, dy, g, p) is None
    assert h.ev == [("usable", "w.slot", True), ("enter", "x", "dy"), ("tuner.run", PKEY + "|s", [winner]),
                    ("notify", "w"), ("exit",)]
    assert narrow == ([winner] if winner != "miopen" else [])
    assert float(h.slots[p].sum()) == (36 * 9 * 64 if winner != "miopen" else 0)


# ---------------------------------------------------------------- fused weight + bias gradient
def _fused(h, cout=256, sinks=True):
    g = NC.geom_pyramid(2, SHAPES, 64, cout)
    x = h.name("x", torch.zeros(2, int(g.M) // 2, 64, dtype=torch.bfloat16))
    dy = h.name("dy", torch.zeros(2, int(g.M) // 2, cout, dtype=torch.bfloat16))
    wp, bp = _Param("w"), _Param("b")
    if sinks:
        h.slot(wp, (cout, 3, 3, 64))
        h.slot(bp, cout)
    return x, dy, g, wp, bp


FKEY = "pwgrad|fused"


def _fused_launch(variant):
    return ("conv_wgrad", "x", "dy", None, variant, "w.slot", True, "b.slot", True)


@pytest.mark.parametrize("usable", [False, True])
def test_fused_bias_taken(monkeypatch, usable):
    h = Harness(monkeypatch, usable=usable, table={FKEY + "|s": "hip23"})
    x, dy, g, wp, bp = _fused(h)
    assert CW.deliver_wgrad_bias_fused(FKEY, x, dy, g, wp, bp)
    run = [_fused_launch(23), ("notify", "w"), ("notify", "b")]
    assert h.ev == [("usable", "w.slot", usable)] + ([("enter", "x", "dy")] + run + [("exit",)] if usable else run)
    assert h.tuner.calls == {FKEY + "|s": 1}


def test_fused_bias_side_is_decided_by_the_weight(monkeypatch):
    h = Harness(monkeypatch, usable=True, table={FKEY + "|s": "hip23"})
    x, dy, g, wp, bp = _fused(h)
    wp.mxr_main_wgrad = True
    assert CW.deliver_wgrad_bias_fused(FKEY, x, dy, g, wp, bp)
    assert h.ev == [("usable", "w.slot", True), _fused_launch(23), ("notify", "w"), ("notify", "b")]


@pytest.mark.parametrize("kw, env", [({"winner": "hip11"}, "1"), ({"winner": "miopen"}, "1"), ({"winner": None}, "1"),
                                     ({"cout": 36 + 2}, "1"), ({"sinks": False}, "1"), ({}, "0")])
def test_fused_bias_fallbacks(monkeypatch, kw, env):
    """The cases of tests/test_fused_bias_dispatch.py: nothing is launched, entered or notified."""
    winner = kw.get("winner", "hip23")
    h = Harness(monkeypatch, usable=True, table={FKEY + "|s": winner} if winner else {})
    monkeypatch.setenv("MXR_WGRAD_FUSED_BIAS", env)
    x, dy, g, wp, bp = _fused(h, cout=kw.get("cout", 256), sinks=kw.get("sinks", True))
    assert not CW.deliver_wgrad_bias_fused(FKEY, x, dy, g, wp, bp)
    assert h.ev == [] and h.tuner.calls == {}


def test_fused_bias_prefers_the_fastest_phase_pipelined_candidate(monkeypatch):
    h = Harness(monkeypatch, table={FKEY + "|s": "hip11"}, prefer=True)
    h.tuner.timings[FKEY + "|s"] = {"hip11": 0.10, "hip23": 0.14, "hip21": 0.12, "hip21~": 0.01, "hip20": "failed",
                                    "hip13": 0.11}
    x, dy, g, wp, bp = _fused(h)
    assert CW.deliver_wgrad_bias_fused(FKEY, x, dy, g, wp, bp)
    assert h.ev == [("prefer", FKEY + "|s", "hip21", dy.numel() * 2 / 4.0e9), ("usable", "w.slot", False),
                    _fused_launch(21), ("notify", "w"), ("notify", "b")]
    h = Harness(monkeypatch, table={FKEY + "|s": "hip11"}, prefer=False)
    h.tuner.timings[FKEY + "|s"] = {"hip11": 0.10, "hip23": 0.14}
    x, dy, g, wp, bp = _fused(h)
    assert not CW.deliver_wgrad_bias_fused(FKEY, x, dy, g, wp, bp)
    assert h.ev == [("prefer", FKEY + "|s", "hip23", dy.numel() * 2 / 4.0e9)]


# ---------------------------------------------------------------- projection dual
def _proj(h, sinks=(True, True), main=False):
    h2 = h.name("h2", torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16))
    x = h.name("x", torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16))
    dy = h.name("dy", torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16))
    s2c, s1 = h.name("sc1", torch.ones(8)), h.name("sc2", torch.ones(8))
    p2c, p1 = _Param("w2c", main), _Param("w1")
    if sinks[0]:
        h.slot(p2c, (8, 1, 1, 8))
    if sinks[1]:
        h.slot(p1, (8, 1, 1, 16))
    return h2, x, dy, 1, s2c, s1, p2c, p1


DKEY = "wgradp|1|4|4|8|16|8|1|4|4|s"
DUAL = ["p8d_0", "p8d_1", "p8d_2", "p8d_4"]


@pytest.mark.parametrize("sinks", [(False, True), (True, False), (False, False)])
def test_proj_missing_sink_runs_nothing(monkeypatch, sinks):
    h = Harness(monkeypatch, usable=True, table={DKEY: "p8d_2"})
    assert CW.run_wgrad_proj(*_proj(h, sinks)) is False
    assert h.ev == []


@pytest.mark.parametrize("usable, main", [(True, False), (False, False), (True, True)])
def test_proj_winner_builds_one_candidate(monkeypatch, usable, main):
    h = Harness(monkeypatch, usable=usable, table={DKEY: "p8d_2"})
    assert CW.run_wgrad_proj(*_proj(h, main=main)) is True
    run = [("tuner.run", DKEY, ["p8d_2"]), ("dual", 2, "w2c.slot", "w1.slot"), ("notify", "w2c"), ("notify", "w1")]
    side = usable and not main
    assert h.ev == [("usable", "w2c.slot", usable)] + (
        [("enter", "h2", "x", "dy", "sc1", "sc2")] + run + [("exit",)] if side else run)


def test_proj_unknown_winner_builds_the_full_set(monkeypatch):
    h = Harness(monkeypatch, table={DKEY: "p8d_3"})
    assert CW.run_wgrad_proj(*_proj(h)) is True
    assert h.ev == [("needs_tuning", DKEY, DUAL), ("usable", "w2c.slot", False), ("tuner.run", DKEY, DUAL),
                    ("dual", 0, "w2c.slot", "w1.slot"), ("notify", "w2c"), ("notify", "w1")]


def test_proj_first_sight_races_on_clones_of_both_slots(monkeypatch):
    h = Harness(monkeypatch, usable=True, tune=True)
    assert CW.run_wgrad_proj(*_proj(h)) is True
    assert h.ev == [("needs_tuning", DKEY, DUAL), ("tuner.run", DKEY, DUAL), ("dual", 0, "clone", "clone"),
                    ("tuner.run", DKEY, DUAL), ("dual", 0, "w2c.slot", "w1.slot"), ("notify", "w2c"), ("notify", "w1")]
    assert h.tuner.calls == {DKEY: 2}


# ---------------------------------------------------------------- bias gradient
@pytest.mark.parametrize("usable", [False, True])
@pytest.mark.parametrize("main", [False, True])
def test_bias_grad_delivery(monkeypatch, usable, main):
    """Side is decided by ``SIDE.usable(dy)`` alone: a ``mxr_main_wgrad`` tag is not consulted."""
    h = Harness(monkeypatch, usable=usable)
    dy = h.name("dy", torch.zeros(2, 5, 40, dtype=torch.bfloat16))
    scale = h.name("scale", torch.ones(36))
    p = _Param("b", main)
    assert CW.deliver_bias_grad(p, dy, scale, channels=36) is h.result
    assert h.ev == [("bias_grad", "dy", "scale", None, False, 36)]
    del h.ev[:]
    h.slot(p, 36)
    assert CW.deliver_bias_grad(p, dy, scale, channels=36) is None
    run = [("bias_grad", "dy", "scale", "b.slot", True, 36), ("notify", "b")]
    assert h.ev == [("usable", "dy", usable)] + ([("enter", "dy", "scale")] + run + [("exit",)] if usable else run)


# ---------------------------------------------------------------- fp8 head weight gradient
def _f8(h):
    g = NC.geom_pyramid(2, SHAPES, 64, 64)
    M = int(g.M)
    f8x = (h.name("xq", torch.zeros(M, 64, dtype=torch.uint8)), h.name("ix", torch.ones(1)))
    f8dy = (h.name("dq", torch.zeros(M, 64, dtype=torch.uint8)), h.name("idq", torch.ones(1)))
    reads = (h.name("x", torch.zeros(1)), h.name("dy", torch.zeros(1)))
    return f8x, f8dy, g, reads


def test_f8_wgrad_without_a_sink_returns_the_tensor(monkeypatch):
    h = Harness(monkeypatch, usable=True)
    f8x, f8dy, g, reads = _f8(h)
    assert F8.deliver_pyramid_wgrad(f8x, f8dy, g, _Param("w"), reads=reads, bias_param=_Param("b")) is h.result
    assert h.ev == [("f8_wgrad", None, None, False, 0, None, False)]


@pytest.mark.parametrize("usable, main", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("bias", ["sink", "no sink", None])
def test_f8_wgrad_delivery(monkeypatch, usable, main, bias):
    h = Harness(monkeypatch, usable=usable)
    monkeypatch.setattr(F8, "WGRAD_VARIANT", 3)
    f8x, f8dy, g, reads = _f8(h)
    wp, bp = _Param("w", main), (_Param("b") if bias else None)
    h.slot(wp, (64, 3, 3, 64))
    if bias == "sink":
        h.slot(bp, 64)
    assert F8.deliver_pyramid_wgrad(f8x, f8dy, g, wp, reads=reads, bias_param=bp) is None
    run = [("f8_wgrad", "w.slot", (64, 3, 3, 64), True, 3, "b.slot" if bias == "sink" else None, True), ("notify", "w")]
    if bias == "sink":
        run.append(("notify", "b"))
    side = usable and not main
    assert h.ev == [("usable", "w.slot", usable)] + (
        [("enter", "xq", "ix", "dq", "idq", "x", "dy")] + run + [("exit",)] if side else run)
