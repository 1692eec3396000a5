"""Checkpoints in the reference's Keras HDF5 layout (plus a fast safetensors format).

Reference behaviour (``/root/reference/train.py:75-78,112-114,404-408``):

* rank 0 writes ``<snapshot_path>/checkpoint-{epoch:02d}.h5`` every epoch (1-based epoch);
* file = ``model.save``: root attrs ``keras_version``, ``backend``, ``model_config``,
  ``training_config``; group ``model_weights`` (attr ``layer_names``; one group per layer with
  attr ``weight_names`` and datasets ``<layer>/<weight>:0``, conv kernels HWIO, BN
  gamma/beta/moving_mean/moving_variance, nested submodels); group ``optimizer_weights``
  (Adam ``iterations``, m, v, vhat placeholders);
* ``--weights`` = ``load_weights(by_name=True, skip_mismatch=True)``; ``--snapshot`` =
  ``models.load_model`` (weights + optimizer).  Unlike the reference, resume also restores the
  epoch (``initial_epoch``) and keeps the DistributedOptimizer.

Internally kernels are OHWI; conversion to/from Keras HWIO happens here.  Writes are atomic
(tmp + rename, in :mod:`.hdf5`).
"""
from __future__ import annotations

import json
import os
import re
import warnings
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import hdf5

KERAS_VERSION = "2.2.4"
FRAMEWORK = "batchai_retinanet_horovod_coco_amd"


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def keras_layers(model) -> "OrderedDict[str, List[Tuple[str, torch.Tensor, str]]]":
    """Ordered Keras layers with weights: layer -> [(weight_name, tensor, kind)].

    kind: 'kernel' (OHWI <-> HWIO), 'oihw' (torch OIHW <-> HWIO), 'dw' (depthwise (C,1,kh,kw) <->
    (kh,kw,C,1)), 'plain'.
    """
    layers: "OrderedDict[str, list]" = OrderedDict()
    if hasattr(model.backbone, "keras_layers"):
        layers.update(model.backbone.keras_layers())

    def conv(c, prefix=""):
        ws = [(prefix + c.keras_name + "/kernel:0", c.weight, "kernel")]
        if c.bias is not None:
            ws.append((prefix + c.keras_name + "/bias:0", c.bias, "plain"))
        return ws

    def bn(b):
        return [(b.keras_name + "/" + n, t, "plain") for n, t in b.keras_weights()]

    bb = model.backbone
    for c in ([] if hasattr(bb, "keras_layers") else bb.convs()):
        layers[c.keras_name] = conv(c)
        if c.bn is not None:
            layers[c.bn.keras_name] = bn(c.bn)
    for c in model.fpn.convs():
        layers[c.keras_name] = conv(c)
    for sub in (model.regression_submodel, model.classification_submodel):
        ws = []
        for c in sub.convs():
            ws.extend(conv(c))
        layers[sub.keras_name] = ws
        # head_norm='gn': each GroupNorm is a layer of its own after its submodel, so files without them still load
        # by name
        for n in (getattr(sub, "norms", None) or []):
            layers[n.keras_name] = [(n.keras_name + "/" + w, t, "plain") for w, t in n.keras_weights()]
    return layers


_GN_LAYER = re.compile(r"^pyramid_(regression|classification)_\d+_gn$")
_GN_TENSOR = re.compile(r"_submodel\.norms\.\d+\.(gamma|beta)$")


def _check_head_norm(path: str, model, file_has_gn: bool, strict: bool = True) -> None:
    """The two cross-loading cases of ``head_norm``: a file without the GroupNorm layers leaves a GN model's gamma /
    beta at their initial values (one warning); a file with them does not load into a model without the norm."""
    model_has_gn = getattr(model, "head_norm", None) == "gn"
    if model_has_gn and not file_has_gn:
        warnings.warn("{} holds no GroupNorm layers: the head towers' gamma / beta stay at their initial values (1 / 0)"
                      .format(path))
    elif file_has_gn and not model_has_gn and strict:
        raise ValueError("{} holds the GroupNorm layers of head towers trained with --head-norm gn, the model has "
                         "none: build it with --head-norm gn (head_norm='gn')".format(path))


def model_config(model) -> Dict:
    cfg = {"class_name": "RetinaNet", "framework": FRAMEWORK,
           "config": {"name": "retinanet", "backbone": model.backbone_name, "num_classes": model.num_classes,
                      "num_anchors": model.num_anchors,
                      "layers": list(keras_layers(model).keys())}}
    if getattr(model, "head_norm", None) is not None:
        # only with the norm on: a default model's config stays what it was
        cfg["config"]["head_norm"] = model.head_norm
        cfg["config"]["head_norm_groups"] = int(model.head_norm_groups)
    if getattr(model, "regression_bins", 0):
        # likewise the distribution box head
        cfg["config"]["regression_bins"] = int(model.regression_bins)
        cfg["config"]["regression_range"] = float(model.regression_range)
    return cfg


# the regression final, the one layer a distribution box head (regression_bins) changes the shape of: its Keras
# weights and its state_dict tensors
_REG_FINAL = re.compile(r"(^|/)pyramid_regression/(kernel|bias):0$|^regression_submodel\.final\.(weight|bias)$")


def stored_regression_bins(path: str) -> Tuple[int, float]:
    """(regression_bins, regression_range) of the model a checkpoint holds: (0, 8.0) for a plain 4-number head."""
    cfg = read_model_config(path).get("config", {})
    return int(cfg.get("regression_bins", 0)), float(cfg.get("regression_range", 8.0))


def _bins_differ(path: str, model) -> bool:
    """Whether the model was built with other ``regression_bins`` than the model the file holds."""
    return stored_regression_bins(path)[0] != int(getattr(model, "regression_bins", 0) or 0)


def stored_dfl_weight(path: str) -> float:
    """The DFL weight a checkpoint was trained with (0.25 unless the file says otherwise)."""
    return float((_stored_training_config(path) or {}).get("dfl_weight", 0.25))


def stored_head_norm(path: str) -> Tuple[Optional[str], int]:
    """(head_norm, head_norm_groups) of the model a checkpoint holds: (None, 32) for one without the norm."""
    cfg = read_model_config(path).get("config", {})
    return cfg.get("head_norm"), int(cfg.get("head_norm_groups", 32))


def optimizer_class(optimizer) -> Optional[str]:
    """The Keras class name of a live optimizer (a ``DistributedOptimizer`` answers for the one it wraps)."""
    if optimizer is None:
        return None
    return getattr(getattr(optimizer, "optimizer", optimizer), "class_name", None) or "Adam"


def _slots(optimizer) -> List[torch.Tensor]:
    """The optimizer's per-parameter state buffers in the order Keras lists them (Adam: m, v; SGD: velocity)."""
    st = optimizer.state_tensors()
    return [st[k] for k in (("m", "v") if optimizer_class(optimizer) == "Adam" else ("velocity",))]


def _stored_training_config(path: str) -> Optional[Dict]:
    if path.endswith(".safetensors"):
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            meta = f.metadata() or {}
        raw = meta.get("training_config")
    else:
        raw = hdf5.File(path, "r").attrs.get("training_config")
        raw = bytes(raw).decode() if raw is not None else None
    return json.loads(raw) if raw else None


def stored_optimizer_class(path: str) -> Optional[str]:
    """The optimizer class a checkpoint was written with (None when it stores no training config)."""
    cfg = _stored_training_config(path)
    if cfg is None:
        return None
    return cfg.get("optimizer_config", {}).get("class_name")


def stored_regression_loss(path: str) -> Optional[str]:
    """The regression loss a checkpoint was trained with -- ``smooth_l1``, ``giou``, ``diou`` or ``ciou`` -- (None
    when it stores no training config)."""
    cfg = _stored_training_config(path)
    name = (cfg or {}).get("loss", {}).get("regression")
    return name.lstrip("_") if name else None


def stored_regression_weight(path: str) -> float:
    """The weight of the regression loss a checkpoint was trained with (1 unless the file says otherwise)."""
    return float((_stored_training_config(path) or {}).get("regression_weight", 1.0))


def stored_classification_loss(path: str) -> Optional[str]:
    """The classification loss a checkpoint was trained with -- ``focal``, ``qfl`` or ``vfl`` -- (None when it stores
    no training config)."""
    cfg = _stored_training_config(path)
    name = (cfg or {}).get("loss", {}).get("classification")
    return name.lstrip("_") if name else None


def stored_assigner(path: str) -> Optional[str]:
    """The target assignment a checkpoint was trained with -- ``iou`` (the fixed thresholds) or ``atss`` -- (None when
    it stores no training config)."""
    cfg = _stored_training_config(path)
    return None if cfg is None else cfg.get("assigner", "iou")


def stored_atss_topk(path: str) -> int:
    """The top-k of the ATSS assignment a checkpoint was trained with (9 unless the file says otherwise)."""
    return int((_stored_training_config(path) or {}).get("atss_topk", 9))


def _class_mismatch(path: str, optimizer) -> bool:
    stored, live = stored_optimizer_class(path), optimizer_class(optimizer)
    if stored is not None and stored != live:
        warnings.warn("{} holds {} state, the live optimizer is {}: weights loaded, optimizer state left fresh"
                      .format(path, stored, live))
        return True
    return False


def training_config(optimizer) -> Dict:
    cfg = optimizer.get_config() if optimizer is not None else {}
    out = {"optimizer_config": {"class_name": optimizer_class(optimizer) or "Adam", "config": cfg},
           # the Trainer marks its optimizer with an IoU regression loss or an IoU-aware classification loss; without
           # one it is the reference's
           "loss": {"regression": "_" + getattr(optimizer, "regression_loss", "smooth_l1"),
                    "classification": "_" + getattr(optimizer, "classification_loss", "focal")},
           "metrics": [], "sample_weight_mode": None, "loss_weights": None}
    if getattr(optimizer, "regression_weight", 1.0) != 1.0:
        out["regression_weight"] = float(optimizer.regression_weight)
    if getattr(optimizer, "assigner", "iou") != "iou":
        # likewise the target assignment: absent for the reference's fixed-threshold rule
        out["assigner"] = optimizer.assigner
        if getattr(optimizer, "atss_topk", 9) != 9:
            out["atss_topk"] = int(optimizer.atss_topk)
    if getattr(optimizer, "dfl_weight", 0.25) != 0.25:
        out["dfl_weight"] = float(optimizer.dfl_weight)
    return out


_TO_KERAS = {"kernel": (1, 2, 3, 0), "oihw": (2, 3, 1, 0), "dw": (2, 3, 0, 1)}
_FROM_KERAS = {"kernel": (3, 0, 1, 2), "oihw": (3, 2, 0, 1), "dw": (2, 3, 0, 1)}


def _to_keras(a: np.ndarray, kind: str) -> np.ndarray:
    return np.transpose(a, _TO_KERAS[kind]) if kind in _TO_KERAS else a


def _from_keras(a: np.ndarray, kind: str) -> np.ndarray:
    if kind in _FROM_KERAS:
        if a.ndim != 4:
            raise ValueError("kernel has rank {}".format(a.ndim))
        return np.transpose(a, _FROM_KERAS[kind])
    return a


def _keras_order_params(model) -> List[Tuple[torch.Tensor, str]]:
    out = []
    for _, ws in keras_layers(model).items():
        for _, t, kind in ws:
            if isinstance(t, torch.nn.Parameter) and t.requires_grad:
                out.append((t, kind))
    return out


def _flat_slice(flat, p):
    seg = flat.by_param[id(p)]
    return seg.offset, seg.numel


EMA_GROUP = "ema_weights"
EMA_PREFIX = "ema/"


def _ema_of(optimizer) -> Optional[torch.Tensor]:
    """The flat weight average of a live optimizer, None when it keeps none (``ema_decay`` 0)."""
    return getattr(optimizer, "ema", None) if optimizer is not None else None


def _ema_view(optimizer, t: torch.Tensor) -> torch.Tensor:
    """The averaged value of ``t`` when it is a trainable parameter of the flat buffer, else ``t`` itself: with this
    the averaged set is a complete weight set."""
    seg = optimizer.flat.by_param.get(id(t))
    if seg is None:
        return t
    return optimizer.ema[seg.offset:seg.offset + seg.numel].view(seg.shape)


def _write_weight_group(g, model, pick=lambda t: t) -> None:
    """A Keras ``model_weights``-layout group: ``layer_names``, per layer ``weight_names`` and the datasets."""
    layers = keras_layers(model)
    hdf5.save_attributes_to_hdf5_group(g, "layer_names", [n.encode() for n in layers])
    g.attrs["backend"] = b"tensorflow"
    g.attrs["keras_version"] = KERAS_VERSION.encode()
    for lname, ws in layers.items():
        lg = g.create_group(lname)
        hdf5.save_attributes_to_hdf5_group(lg, "weight_names", [w[0].encode() for w in ws])
        for wname, t, kind in ws:
            a = _to_keras(_np(pick(t)), kind)
            lg.create_dataset(wname, data=a.astype(np.float32))


def _ema_missing(path: str, optimizer) -> None:
    """A snapshot without an averaged set, loaded into a run that keeps one: the average starts from the weights
    (one warning per load)."""
    warnings.warn("{} holds no averaged weights ({}): the weight EMA starts from the loaded weights"
                  .format(path, EMA_GROUP))
    optimizer.seed_ema()


def _restore_ema_h5(f, path: str, model, optimizer) -> None:
    if _ema_of(optimizer) is None:
        return                      # a run without --ema-decay ignores a stored average
    if EMA_GROUP not in f:
        _ema_missing(path, optimizer)
        return
    g = f[EMA_GROUP]
    flat = optimizer.flat
    with torch.no_grad():
        for lname, ws in keras_layers(model).items():
            if lname not in g and _GN_LAYER.match(lname):
                continue            # GroupNorm layers the file does not hold: their average stays the weights
            for wname, t, kind in ws:
                seg = flat.by_param.get(id(t))
                if seg is None:
                    continue
                a = _from_keras(np.asarray(g[lname][wname]), kind)
                optimizer.ema[seg.offset:seg.offset + seg.numel].copy_(
                    torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(optimizer.ema.device))
    optimizer.ema_start = int(optimizer.iterations) - int(np.asarray(g.attrs["ema_updates"]).reshape(-1)[0])


def save_keras_h5(path: str, model, optimizer=None, epoch: Optional[int] = None, include_optimizer: bool = True) -> str:
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with hdf5.File(path, "w") as f:
        f.attrs["keras_version"] = KERAS_VERSION.encode()
        f.attrs["backend"] = b"tensorflow"
        f.attrs["model_config"] = json.dumps(model_config(model)).encode()
        if optimizer is not None:
            f.attrs["training_config"] = json.dumps(training_config(optimizer)).encode()
        if epoch is not None:
            f.attrs["epoch"] = np.int64(epoch)
        _write_weight_group(f.create_group("model_weights"), model)
        if include_optimizer and _ema_of(optimizer) is not None:
            # the averaged set, laid out like model_weights (trainable tensors averaged, the others as they are)
            eg = f.create_group(EMA_GROUP)
            _write_weight_group(eg, model, lambda t: _ema_view(optimizer, t))
            eg.attrs["ema_decay"] = np.float64(optimizer.ema_decay)
            eg.attrs["ema_updates"] = np.int64(optimizer.ema_updates)
        if include_optimizer and optimizer is not None and hasattr(optimizer, "m"):
            ow = f.create_group("optimizer_weights")
            params = _keras_order_params(model)
            names = ["Adam/iterations:0"]
            ow.create_dataset("Adam/iterations:0", data=np.array(int(optimizer.iterations), dtype=np.int64))
            n = len(params)
            flat = optimizer.flat
            for slot, buf in (("m", optimizer.m), ("v", optimizer.v)):
                for i, (p, kind) in enumerate(params):
                    idx = i if slot == "m" else n + i
                    name = "training/Adam/Variable{}:0".format("" if idx == 0 else "_{}".format(idx))
                    off, num = _flat_slice(flat, p)
                    a = _to_keras(buf[off:off + num].detach().cpu().numpy().reshape(p.shape), kind)
                    ow.create_dataset(name, data=a)
                    names.append(name)
            for i in range(n):
                name = "training/Adam/Variable_{}:0".format(2 * n + i)
                ow.create_dataset(name, data=np.zeros((1,), dtype=np.float32))
                names.append(name)
            hdf5.save_attributes_to_hdf5_group(ow, "weight_names", [x.encode() for x in names])
        elif include_optimizer and optimizer is not None and optimizer_class(optimizer) == "SGD":
            ow = f.create_group("optimizer_weights")
            names = ["SGD/iterations:0"]
            ow.create_dataset(names[0], data=np.array(int(optimizer.iterations), dtype=np.int64))
            flat, buf = optimizer.flat, _slots(optimizer)[0]
            for i, (p, kind) in enumerate(_keras_order_params(model)):
                name = "training/SGD/Variable{}:0".format("" if i == 0 else "_{}".format(i))
                off, num = _flat_slice(flat, p)
                ow.create_dataset(name, data=_to_keras(buf[off:off + num].detach().cpu().numpy().reshape(p.shape), kind))
                names.append(name)
            hdf5.save_attributes_to_hdf5_group(ow, "weight_names", [x.encode() for x in names])
    return path


def _layer_weights_from_file(f, group: str = "model_weights") -> "OrderedDict[str, List[Tuple[str, np.ndarray]]]":
    if group in f:
        root = f[group]
    elif group == "model_weights":
        root = f                    # a weights-only file
    else:
        raise ValueError("the file holds no group '{}'".format(group))
    names = hdf5.load_attributes_from_hdf5_group(root, "layer_names")
    out = OrderedDict()
    for ln in names:
        g = root[ln]
        wn = hdf5.load_attributes_from_hdf5_group(g, "weight_names")
        out[ln] = [(w, np.asarray(g[w])) for w in wn]
    return out


def has_ema_weights(path: str) -> bool:
    """Whether a checkpoint holds an averaged weight set (group ``ema_weights`` / tensors under ``ema/``)."""
    if path.endswith(".safetensors"):
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            return any(k.startswith(EMA_PREFIX) for k in f.keys())
    return EMA_GROUP in hdf5.File(path, "r")


def load_weights(model, path: str, by_name: bool = True, skip_mismatch: bool = False,
                 group: str = "model_weights", strict_head_norm: bool = True,
                 skip_regression_final: bool = False) -> List[str]:
    """Keras ``load_weights`` (HDF5 or safetensors).  Returns the list of skipped weights.  ``group="ema_weights"``
    loads the averaged set a run with a weight EMA stored; a ValueError when the file has none.
    ``skip_regression_final``: the regression final's kernel and bias stay at their initial values where the file's
    have another shape (a model built with other ``regression_bins`` than the file's)."""
    if group not in ("model_weights", EMA_GROUP):
        raise ValueError("group must be 'model_weights' or '{}', got {!r}".format(EMA_GROUP, group))
    if path.endswith(".safetensors"):
        return load_safetensors(model, path, optimizer=None, skip_mismatch=skip_mismatch,
                                prefix=EMA_PREFIX if group == EMA_GROUP else "", strict_head_norm=strict_head_norm,
                                skip_regression_final=skip_regression_final)[1]
    f = hdf5.File(path, "r")
    file_layers = _layer_weights_from_file(f, group)
    layers = keras_layers(model)
    if by_name:
        _check_head_norm(path, model, any(_GN_LAYER.match(l) for l in file_layers), strict_head_norm)
    skipped = []
    if not by_name:
        wl = [l for l in layers if layers[l]]
        fl = [l for l in file_layers if file_layers[l]]
        if len(wl) != len(fl):
            raise ValueError("You are trying to load a weight file containing {} layers into a model with {} layers."
                             .format(len(fl), len(wl)))
        pairs = list(zip(wl, fl))
    else:
        pairs = [(l, l) for l in layers if l in file_layers]
    with torch.no_grad():
        for mine, theirs in pairs:
            ws, fws = layers[mine], file_layers[theirs]
            if len(ws) != len(fws):
                msg = "Layer '{}' expects {} weights, but the saved weights have {} elements.".format(mine, len(ws),
                                                                                                  len(fws))
                if skip_mismatch:
                    skipped.append(mine)
                    continue
                raise ValueError(msg)
            for (wname, t, kind), (fname, arr) in zip(ws, fws):
                a = _from_keras(arr, kind)
                if tuple(a.shape) != tuple(t.shape):
                    if skip_mismatch or (skip_regression_final and _REG_FINAL.search(wname)):
                        skipped.append(wname)
                        continue
                    raise ValueError("Layer '{}' weight shape {} does not match saved shape {}".format(
                        mine, tuple(t.shape), tuple(a.shape)))
                t.data.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(t.device, t.dtype))
    return skipped


def load_optimizer_h5(model, optimizer, path: str) -> bool:
    """Restore the optimizer state a Keras-layout file holds.  False (state untouched) when the file has none, or
    holds another optimizer class's: slots are never matched by position across classes."""
    f = hdf5.File(path, "r")
    if "optimizer_weights" not in f:
        return False
    if _class_mismatch(path, optimizer):
        return False
    ow = f["optimizer_weights"]
    names = hdf5.load_attributes_from_hdf5_group(ow, "weight_names")
    params = _keras_order_params(model)
    n = len(params)
    slots = _slots(optimizer)
    if len(names) < 1 + len(slots) * n or not names[0].startswith(optimizer_class(optimizer) + "/"):
        return False
    # slots are matched by position: a file written for another list of trainable parameters (a model with or without
    # the head towers' GroupNorm layers) holds none for this model -- judged before anything is touched
    stored = 3 if optimizer_class(optimizer) == "Adam" else 1          # Adam: m, v and the vhat placeholders
    fits = len(names) == 1 + stored * n
    for k in range(len(slots) if fits else 0):
        for i, (p, kind) in enumerate(params):
            shape = tuple(ow[names[1 + k * n + i]].shape)
            want = tuple(p.shape[j] for j in _TO_KERAS[kind]) if kind in _TO_KERAS else tuple(p.shape)
            fits = fits and shape == want
    if not fits:
        warnings.warn("{} holds optimizer state for another list of trainable parameters than the model's: weights "
                      "loaded, optimizer state left fresh".format(path))
        return False
    optimizer.iterations = int(np.asarray(ow[names[0]]).reshape(-1)[0])
    flat = optimizer.flat
    with torch.no_grad():
        for k, buf in enumerate(slots):
            for i, (p, kind) in enumerate(params):
                idx = 1 + k * n + i
                a = _from_keras(np.asarray(ow[names[idx]]), kind)
                off, num = _flat_slice(flat, p)
                buf[off:off + num].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(buf.device))
    _restore_ema_h5(f, path, model, optimizer)
    return True


def read_model_config(path: str) -> Dict:
    if path.endswith(".safetensors"):
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            meta = f.metadata() or {}
        return json.loads(meta.get("model_config", "{}"))
    f = hdf5.File(path, "r")
    raw = f.attrs.get("model_config")
    return json.loads(bytes(raw).decode()) if raw is not None else {}


def checkpoint_epoch(path: str) -> Optional[int]:
    """Epoch stored in the checkpoint (attribute), else parsed from ``checkpoint-NN``."""
    try:
        if path.endswith(".safetensors"):
            from safetensors import safe_open
            with safe_open(path, framework="pt") as f:
                meta = f.metadata() or {}
            if "epoch" in meta:
                return int(meta["epoch"])
        else:
            f = hdf5.File(path, "r")
            if "epoch" in f.attrs:
                return int(np.asarray(f.attrs["epoch"]).reshape(-1)[0])
    except Exception:  # noqa: BLE001
        pass
    m = re.search(r"(\d+)\.(h5|safetensors)$", os.path.basename(path))
    return int(m.group(1)) if m else None


def load_model(filepath: str, backbone_name: str = "resnet50", **kwargs):
    """``models.load_model``: rebuild the architecture from the stored config, load weights.  ``head_norm`` /
    ``head_norm_groups`` and ``regression_bins`` / ``regression_range`` given here win over the stored ones (the
    weights they have in common are loaded)."""
    from .. import models
    cfg = read_model_config(filepath).get("config", {})
    name = cfg.get("backbone", backbone_name)
    norm = {}
    head_norm = kwargs["head_norm"] if "head_norm" in kwargs else cfg.get("head_norm")
    if head_norm not in (None, "none"):
        norm = dict(head_norm=head_norm,
                    head_norm_groups=int(kwargs.get("head_norm_groups") or cfg.get("head_norm_groups", 32)))
    # likewise ``regression_bins`` / ``regression_range``: every layer but the regression final is shared
    stored_bins = int(cfg.get("regression_bins", 0))
    bins = int(kwargs["regression_bins"]) if kwargs.get("regression_bins") is not None else stored_bins
    if bins:
        rng = kwargs.get("regression_range")
        norm.update(regression_bins=bins,
                    regression_range=float(rng if rng is not None else cfg.get("regression_range", 8.0)))
    model = models.backbone(name).retinanet(int(cfg.get("num_classes", kwargs.get("num_classes", 80))), **norm)
    if bins != stored_bins:
        warnings.warn("{} holds a regression final for {}, the model is built with {}: that layer stays at its initial "
                      "values, every other layer is loaded".format(filepath, _bins_name(stored_bins), _bins_name(bins)))
    load_weights(model, filepath, by_name=True, skip_mismatch=False, strict_head_norm="head_norm" not in kwargs,
                 skip_regression_final=bins != stored_bins)
    return model


def _bins_name(bins: int) -> str:
    return "{} bins per box side".format(bins) if bins else "4 numbers per box"


# ------------------------------------------------------------------------------ safetensors
def save_safetensors(path: str, model, optimizer=None, epoch: Optional[int] = None) -> str:
    from safetensors.torch import save_file
    tensors = {k: v.detach().contiguous().cpu() for k, v in model.state_dict().items()}
    meta = {"model_config": json.dumps(model_config(model)), "framework": FRAMEWORK}
    if epoch is not None:
        meta["epoch"] = str(int(epoch))
    if optimizer is not None and hasattr(optimizer, "m"):
        tensors["__optimizer__.m"] = optimizer.m.detach().cpu()
        tensors["__optimizer__.v"] = optimizer.v.detach().cpu()
        meta["iterations"] = str(int(optimizer.iterations))
        meta["lr"] = repr(float(optimizer.lr))
        meta["training_config"] = json.dumps(training_config(optimizer))
    elif optimizer is not None and optimizer_class(optimizer) == "SGD":
        tensors["__optimizer__.velocity"] = _slots(optimizer)[0].detach().cpu()
        meta["iterations"] = str(int(optimizer.iterations))
        meta["lr"] = repr(float(optimizer.lr))
        meta["training_config"] = json.dumps(training_config(optimizer))
    if _ema_of(optimizer) is not None:
        params = dict(model.named_parameters())
        for k, v in model.state_dict().items():
            t = _ema_view(optimizer, params[k]) if k in params else v
            tensors[EMA_PREFIX + k] = t.detach().contiguous().cpu().clone()
        meta["ema_decay"] = repr(float(optimizer.ema_decay))
        meta["ema_updates"] = str(int(optimizer.ema_updates))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    save_file(tensors, tmp, metadata=meta)
    os.replace(tmp, path)
    return path


def load_safetensors(model, path: str, optimizer=None, skip_mismatch: bool = False, prefix: str = "",
                     strict_head_norm: Optional[bool] = True, skip_regression_final: bool = False):
    """Returns (metadata, skipped tensors); ``metadata["optimizer_restored"]`` tells whether the optimizer state was
    restored (only from a file written with the live optimizer's class).  ``prefix="ema/"`` loads the averaged set.
    ``skip_regression_final``: as in :func:`load_weights`."""
    from safetensors.torch import load_file
    from safetensors import safe_open
    sd = load_file(path)
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
    if prefix:
        if not any(k.startswith(prefix) for k in sd):
            raise ValueError("the file holds no tensors under '{}'".format(prefix))
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    own = model.state_dict()
    skipped = []
    file_has_gn = any(_GN_TENSOR.search(k) for k in sd)
    if strict_head_norm is not None:
        _check_head_norm(path, model, file_has_gn, strict_head_norm)
    with torch.no_grad():
        for k, v in own.items():
            if not file_has_gn and _GN_TENSOR.search(k):
                continue            # stays at its initial value (_check_head_norm)
            if k not in sd or tuple(sd[k].shape) != tuple(v.shape):
                if skip_mismatch or (skip_regression_final and k in sd and _REG_FINAL.search(k)):
                    skipped.append(k)
                    continue
                raise ValueError("missing or mismatched tensor {}".format(k))
            v.copy_(sd[k].to(v.device, v.dtype))
        restored = False
        if optimizer is not None and not _class_mismatch(path, optimizer):
            state = {k: t for k, t in optimizer.state_tensors().items() if k != "ema"}     # the average: below
            keys = ["__optimizer__." + k for k in state]
            if all(k in sd and sd[k].numel() == t.numel() for k, t in zip(keys, state.values())):
                for k, t in zip(keys, state.values()):
                    t.copy_(sd[k].to(t.device))
                optimizer.iterations = int(meta.get("iterations", 0))
                if "lr" in meta:
                    optimizer.lr = float(meta["lr"])
                restored = True
            elif skip_regression_final and all(k in sd for k in keys):
                # the flat state of a model with another regression final: no slot of it lines up with this one's
                warnings.warn("{} holds optimizer state for another list of trainable parameters than the model's: "
                              "weights loaded, optimizer state left fresh".format(path))
            if restored:
                if _ema_of(optimizer) is not None:
                    params = dict(model.named_parameters())
                    if all(EMA_PREFIX + k in sd for k in params) and "ema_updates" in meta:
                        for k, prm in params.items():
                            seg = optimizer.flat.by_param.get(id(prm))
                            if seg is not None:
                                optimizer.ema[seg.offset:seg.offset + seg.numel].copy_(
                                    sd[EMA_PREFIX + k].reshape(-1).to(optimizer.ema.device))
                        optimizer.ema_start = optimizer.iterations - int(meta["ema_updates"])
                    else:
                        _ema_missing(path, optimizer)
    meta = dict(meta, optimizer_restored=restored)
    return meta, skipped


def save_checkpoint(path: str, model, optimizer=None, epoch: Optional[int] = None, fmt: str = "h5") -> str:
    if fmt == "safetensors" or path.endswith(".safetensors"):
        return save_safetensors(path, model, optimizer, epoch)
    return save_keras_h5(path, model, optimizer, epoch)


def load_optimizer(model, optimizer, path: str) -> bool:
    """Optimizer state from a checkpoint of either format; False when the file holds none for this optimizer class
    (a safetensors file's weights are read again on the way)."""
    if path.endswith(".safetensors"):
        # (the second read of a file whose weights load_weights has judged: no second head_norm warning)
        return bool(load_safetensors(model, path, optimizer, strict_head_norm=None,
                                     skip_regression_final=_bins_differ(path, model))[0]["optimizer_restored"])
    return load_optimizer_h5(model, optimizer, path)


def restore_checkpoint(path: str, model, optimizer=None) -> Optional[int]:
    """Weights (+ optimizer state when present).  Returns the stored epoch."""
    if path.endswith(".safetensors"):
        load_safetensors(model, path, optimizer)
    else:
        load_weights(model, path, by_name=True)
        if optimizer is not None:
            load_optimizer_h5(model, optimizer, path)
    return checkpoint_epoch(path)
