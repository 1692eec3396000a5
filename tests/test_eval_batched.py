"""Batched, rank-sharded evaluation (eval/batched.py) on the CPU: the sharding plan, equality with the per-image
path through a stub model, the gather's checks, and the CocoEval callback at world 2 over gloo."""
import json
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from eval_batched_common import MAX_SIDE, MIN_SIDE, N_IMAGES, SIZES, StubModel, legacy_rows, make_generator, write_fixture


@pytest.fixture(scope="module")
def fixture_root(tmp_path_factory):
    return write_fixture(tmp_path_factory.mktemp("coco_eval_fixture"))


# ------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("pad", [0, 32])
@pytest.mark.parametrize("batch_size", [1, 4])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 7, 10])
def test_plan_batches(n, world, batch_size, pad):
    from batchai_retinanet_horovod_coco_amd.data.generator import pad_shape
    from batchai_retinanet_horovod_coco_amd.eval.batched import plan_batches, resized_hw
    hws = [SIZES[(i + i // 2) % 3] for i in range(n)]
    hws = [(h + (i % 2) * 40, w) for i, (h, w) in enumerate(hws)]            # a few more shapes
    plan = plan_batches(hws, batch_size, MIN_SIDE, MAX_SIDE, pad, world)
    assert len(plan) == world
    seen = [i for rank in plan for batch in rank for i in batch]
    assert sorted(seen) == list(range(n))                                    # every index exactly once
    for rank in plan:
        for batch in rank:
            assert 1 <= len(batch) <= batch_size
            keys = {tuple(pad_shape(resized_hw(hws[i], MIN_SIDE, MAX_SIDE), pad)) for i in batch}
            assert len(keys) == 1
    # every rank computes the plan for itself from the same arguments: it must not depend on anything else
    assert plan_batches(list(hws), batch_size, MIN_SIDE, MAX_SIDE, pad, world) == plan
    whole = plan_batches(hws, batch_size, MIN_SIDE, MAX_SIDE, pad, 1)[0]
    assert all(plan[r] == whole[r::world] for r in range(world))             # batch j belongs to rank j % world


def test_plan_pad_merges_shapes():
    from batchai_retinanet_horovod_coco_amd.eval.batched import plan_batches
    hws = [(96, 128), (100, 128), (96, 128), (100, 128)]     # resized 64x85 and 64x82: one 64x96 class at pad 32
    assert plan_batches(hws, 4, MIN_SIDE, MAX_SIDE, 0, 1) == [[[1, 3], [0, 2]]]
    assert plan_batches(hws, 4, MIN_SIDE, MAX_SIDE, 32, 1) == [[[0, 1, 2, 3]]]
    assert plan_batches(hws, 4, MIN_SIDE, MAX_SIDE, 0, 2) == [[[1, 3]], [[0, 2]]]


# ------------------------------------------------------------------------------------------ stub model
@pytest.fixture(scope="module")
def legacy(fixture_root):
    """Per-image results of the stub model: computed once, shared, never modified."""
    from batchai_retinanet_horovod_coco_amd.eval.coco_eval import predict_image
    gen, model = make_generator(fixture_root), StubModel()
    return [legacy_rows(*predict_image(gen, model, i)) for i in range(gen.size())]


@pytest.mark.parametrize("pad", [0, 32])
def test_collect_equals_per_image(fixture_root, legacy, pad):
    from batchai_retinanet_horovod_coco_amd.eval.batched import collect_detections
    gen, model = make_generator(fixture_root), StubModel()
    got = collect_detections(gen, model, 4, pad_multiple=pad, workers=2)
    assert sorted(got) == list(range(N_IMAGES))
    assert any(len(v[1]) for v in got.values()) and any(len(v[1]) < StubModel.D for v in got.values())
    for i in range(N_IMAGES):
        for a, b in zip(got[i], legacy[i]):
            assert np.array_equal(a, b), (i, a, b)
    assert max(c[0] for c in model.calls) > 1                       # really batched
    if pad == 0:
        assert {c[1:3] for c in model.calls} == {(64, 85), (85, 64), (64, 64)}
    else:
        assert {c[1:3] for c in model.calls} == {(64, 96), (96, 64), (64, 64)}


def test_collect_without_pool(fixture_root, legacy):
    from batchai_retinanet_horovod_coco_amd.eval.batched import collect_detections
    got = collect_detections(make_generator(fixture_root), StubModel(), 3, workers=0)
    for i in range(N_IMAGES):
        for a, b in zip(got[i], legacy[i]):
            assert np.array_equal(a, b)


def test_image_hw_sources(fixture_root):
    from batchai_retinanet_horovod_coco_amd.eval.batched import image_hw
    gen = make_generator(fixture_root)
    want = [gen.load_image(i).shape[:2] for i in range(gen.size())]
    assert [image_hw(gen, i) for i in range(gen.size())] == want

    class PathOnly:
        image_path = gen.image_path

    class LoadOnly:
        load_image = gen.load_image
    assert [image_hw(PathOnly(), i) for i in range(gen.size())] == want
    assert [image_hw(LoadOnly(), i) for i in range(gen.size())] == want


def _stats_and_files(fixture_root, path, **kw):
    from batchai_retinanet_horovod_coco_amd.eval.coco_eval import evaluate_coco
    stats = evaluate_coco(make_generator(fixture_root), StubModel(), results_path=str(path), verbose=False, **kw)
    with open(path) as f:
        results = json.load(f)
    with open(str(path).replace("_bbox_results.json", "") + "_processed_image_ids.json") as f:
        ids = json.load(f)
    return stats, results, ids


def test_evaluate_coco_equal(fixture_root, tmp_path):
    s0, r0, i0 = _stats_and_files(fixture_root, tmp_path / "a_bbox_results.json")
    s1, r1, i1 = _stats_and_files(fixture_root, tmp_path / "b_bbox_results.json", batch_size=4)
    assert s0 is not None and len(s0) == 12 and len(r0) > 0
    np.testing.assert_allclose(s1, s0, rtol=0, atol=0)
    assert r1 == r0 and i1 == i0
    with open(tmp_path / "a_bbox_results.json") as a, open(tmp_path / "b_bbox_results.json") as b:
        assert a.read() == b.read()


def test_voc_evaluate_equal(fixture_root):
    from batchai_retinanet_horovod_coco_amd.eval import voc_eval
    a = voc_eval.evaluate(make_generator(fixture_root), StubModel())
    b = voc_eval.evaluate(make_generator(fixture_root), StubModel(), batch_size=4, pad_multiple=32, workers=1)
    assert a == b and any(n > 0 for _, n in a.values())


# ------------------------------------------------------------------------------------------ gather
def _det(k):
    return (np.zeros((k, 4), np.float32), np.zeros(k, np.float32), np.zeros(k, np.int32))


def test_gather_world1_returns_argument():
    from batchai_retinanet_horovod_coco_amd.eval import batched
    local = {0: _det(1)}
    assert batched.gather_detections(local) is local


@pytest.mark.parametrize("parts,size,what", [
    ([{0: _det(1), 1: _det(2)}, {1: _det(2), 2: _det(0)}], 3, "twice [1]"),
    ([{0: _det(1)}, {2: _det(0)}], 3, "missing [1]"),
    ([{0: _det(1)}, {1: _det(0)}], 3, "missing [2]"),
    ([{0: _det(1)}, {2: _det(0)}], None, "missing [1]"),
])
def test_gather_raises(monkeypatch, parts, size, what):
    from batchai_retinanet_horovod_coco_amd.eval import batched
    monkeypatch.setattr(batched, "_world", lambda: (1, 2))
    monkeypatch.setattr(batched.collectives, "allgather_object", lambda obj: parts)
    with pytest.raises(RuntimeError, match=what.replace("[", r"\[").replace("]", r"\]")):
        batched.gather_detections(parts[1], size)


def test_gather_merges(monkeypatch):
    from batchai_retinanet_horovod_coco_amd.eval import batched
    parts = [{0: _det(1), 2: _det(3)}, {1: _det(2)}]
    monkeypatch.setattr(batched, "_world", lambda: (0, 2))
    monkeypatch.setattr(batched.collectives, "allgather_object", lambda obj: parts)
    merged = batched.gather_detections(parts[0], 3)
    assert sorted(merged) == [0, 1, 2] and [len(merged[i][1]) for i in range(3)] == [1, 2, 3]


# ------------------------------------------------------------------------------------------ gloo, world 2
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _w_callback(rank, world, port, root, out):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "LOCAL_WORLD_SIZE": str(world)})
    from batchai_retinanet_horovod_coco_amd.parallel import runtime
    runtime.init(backend="gloo", device="cpu", timeout_s=60)
    from batchai_retinanet_horovod_coco_amd.eval.callbacks import CocoEval
    cwd = os.path.join(out, "cwd{}".format(rank))
    os.makedirs(cwd)
    os.chdir(cwd)                                     # the result files go to the working directory
    model = StubModel()
    cb = CocoEval(make_generator(root), batch_size=3, workers=1)
    cb.set_model(model)
    logs = {}
    cb.on_epoch_end(0, logs)
    torch.save({"logs": logs, "files": sorted(os.listdir(cwd)), "images": sum(c[0] for c in model.calls)},
               os.path.join(out, "r{}.pt".format(rank)))
    runtime.shutdown()


def test_coco_eval_callback_world2(fixture_root, tmp_path):
    from batchai_retinanet_horovod_coco_amd.eval.coco_eval import STAT_NAMES
    want, _, _ = _stats_and_files(fixture_root, tmp_path / "w1_bbox_results.json")
    out = tempfile.mkdtemp()
    mp.spawn(_w_callback, args=(2, _port(), fixture_root, out), nprocs=2, join=True)     # both ranks return
    r = [torch.load(os.path.join(out, "r{}.pt".format(k)), weights_only=False) for k in range(2)]
    for k in range(2):
        assert sorted(r[k]["logs"]) == sorted(STAT_NAMES)
        np.testing.assert_allclose([r[k]["logs"][n] for n in STAT_NAMES], want, rtol=0, atol=0)
    assert r[0]["files"] == ["val2017_bbox_results.json", "val2017_processed_image_ids.json"]
    assert r[1]["files"] == []                                                       # rank 1 writes nothing
    assert r[0]["images"] + r[1]["images"] == N_IMAGES and min(r[0]["images"], r[1]["images"]) > 0
