"""Evaluation: COCO bbox COCOeval re-implementation, VOC-style mAP, evaluation callbacks, and the batched,
rank-sharded detection collection behind ``--eval-batch-size`` (``batched.py``)."""
