"""Tree ensembles of 17 to 256 classes on the class-tile kernel (``ops/csrc/tree_classes.hip``).

:class:`~flink_jpmml_amd.runtime.plans.TreePlan`'s kernels keep ``C x 256`` LDS accumulators and stop
at 16 class slots. :class:`ClassForestPlan` lowers the same binary-form :class:`EnsembleSpec` for a
kernel that tiles classes and rows (64 rows, up to 256 class planes in LDS):

* majority votes (``mode="class"``) and K-class boosted chains (``mode="slot"``) as PAIR leaves,
  one ``{class slot, value}`` pair per leaf: a vote carries its tree's weight, a chain tree its
  weighted leaf value; the chain intercepts start the accumulators (``acc_init``);
* probability leaves (``P == C``: averaging forests, single classification trees) as DENSE leaves,
  one weight-scaled row of ``Cp`` floats per leaf.

``compile_plan`` builds it when, and only when, ``TreePlan`` refuses an ensemble for its class count.
"""

from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

from .plans import (EPI_ARGMAX, EPI_SOFTMAX, DevicePlan, NotLowerable, TreePlan, _addr, _epilogue, _label_table,
                    ensemble_spec)

MAX_CLASSES = 256  # csrc/tree_classes.hip: CLS_MAX, CLS_STAGE_MAX, CR, CCHUNK
MAX_STAGE = 256
TILE_ROWS = 64
CHUNK_TREES = 32
LDS_BYTES = 160 * 1024  # one gfx950 CU


def lds_bytes(n_stage: int, Cp: int) -> int:
    """LDS of one workgroup: feature planes, class accumulators, two hit tables, the rejected rows."""
    return (n_stage + Cp) * TILE_ROWS * 4 + 2 * CHUNK_TREES * TILE_ROWS * 4 + TILE_ROWS * 4


class ClassForestPlan(TreePlan):
    """A classification tree ensemble of up to 256 classes: the same labels, label table and
    epilogue as :class:`TreePlan`, scored by ``pmml_tree_classes_launch``."""

    kind = "tree_classes"
    _STATE = DevicePlan._STATE + ("depth", "n_trees", "layout", "P", "C", "Cp", "dense", "n_stage", "blob", "leaves",
                                  "roots", "feat_map", "acc_init", "table", "labels", "epi_args", "full_epi", "has_dr")

    def __init__(self, compiled, device, precision: str = "fp32", tree_shard=None, layout: str = "auto", **_):
        DevicePlan.__init__(self, compiled, device)  # not TreePlan's: its lowering stops at 16 class slots
        from .hybrid import pack_trees

        if precision == "fp8":
            raise NotLowerable("fp8 leaves need the PERFECT layout")
        if tree_shard is not None:
            raise NotLowerable("tree sharding supports single-score ensembles (regression / binary chains)")
        if layout not in ("auto", "classes"):
            raise NotLowerable(f"the class-tile kernel has one layout, not {layout!r}")
        spec = ensemble_spec(compiled, max_chain_classes=MAX_CLASSES)  # NotBinaryForm: general trees stay at 16
        if spec.labels is None or spec.epi.get("mode") not in (EPI_ARGMAX, EPI_SOFTMAX):
            raise NotLowerable("the class-tile kernel scores classification ensembles")
        if spec.C > MAX_CLASSES:
            raise NotLowerable(f"{spec.C} class slots: the class-tile kernel accumulates at most {MAX_CLASSES}")
        pair = spec.mode in ("class", "slot")
        if not pair and not (spec.mode == "sum" and spec.P == spec.C and spec.slots is None):
            raise NotLowerable("the class-tile kernel takes votes, class slots or P == C probability leaves")
        stage = self._stage_columns(compiled, spec.trees)
        if len(stage) > MAX_STAGE:
            raise NotLowerable(f"{len(stage)} staged columns: the class-tile kernel holds at most {MAX_STAGE}")
        self.layout, self.spec = "classes", spec
        self.full_epi, self.epi_args, self.labels = dict(spec.epi), dict(spec.epi), spec.labels
        self.n_trees, self.P, self.C = len(spec.trees), spec.P, spec.C
        self.Cp = -(-spec.C // 16) * 16  # every class quarter is whole float4s of a DENSE leaf row
        self.dense, self.n_stage = 0 if pair else 1, len(stage)
        self.depth = max(1, max(t.depth for t in spec.trees))
        need = lds_bytes(self.n_stage, self.Cp)
        if need > LDS_BYTES:
            raise NotLowerable(f"{self.n_stage} staged columns x {spec.C} classes need {need} bytes of LDS "
                               f"> {LDS_BYTES}")
        # nodes of the pointer packer over the staged column numbering; a node's feature field
        # becomes the byte offset of its [64]-row plane
        col = {f: j for j, f in enumerate(stage)}
        trees = [dataclasses.replace(t, feature=np.array([col[int(f)] if f >= 0 else -1 for f in t.feature]))
                 for t in spec.trees]
        P = 1 if pair else spec.P
        # (a vote leaf holds its class index: no weight; chain and probability leaves are weighted here)
        weights = [1.0] * len(trees) if spec.mode == "class" else spec.weights
        _, nodes, leaves, roots, self.has_dr = pack_trees(trees, weights, P, 0, False)
        meta = nodes[:, 1]
        nodes[:, 1] = (meta & np.uint32(0xFFFF0000)) | ((meta & np.uint32(0xFFFF)) * np.uint32(TILE_ROWS * 4))
        per_tree = np.array([int((t.feature < 0).sum()) for t in spec.trees])  # the packer's leaves, tree by tree
        owner = np.repeat(np.arange(len(trees)), per_tree)
        if pair:
            lv = leaves[:, 0].astype(np.float64)
            if spec.mode == "class":  # leaf = class index (NaN: no class), value = the tree's vote
                w = np.asarray(spec.tree_w or [1.0] * len(trees), dtype=np.float64)[owner]
                slot = np.where(np.isnan(lv), -1, np.nan_to_num(lv)).astype(np.int32)
                if (slot >= spec.C).any():
                    raise NotLowerable("a vote leaf names a class outside the ensemble's")
                if (slot < 0).any() and compiled.evaluator.mm.missing_prediction_treatment == "skipSegment":
                    raise NotLowerable("skipSegment over leaves without a class is host-only")
                val = w
            else:  # a chain tree adds weight x leaf to its class slot
                slot, val = np.asarray(spec.slots, dtype=np.int32)[owner], lv
            table = np.stack([slot, val.astype(np.float32).view(np.int32)], axis=1)
            self.leaves = self._t(np.ascontiguousarray(table, dtype=np.int32).reshape(-1))
        else:
            rows = np.zeros((leaves.shape[0], self.Cp), dtype=np.float32)
            rows[:, :spec.C] = leaves
            self.leaves = self._t(rows.reshape(-1))
        self.blob = self._t(nodes.reshape(-1).view(np.int32))
        self.roots = self._t(roots)
        self.feat_map = self._t(np.asarray(stage, dtype=np.int32))
        init = spec.acc_init
        self.acc_init = self._t(np.asarray(init, dtype=np.float32)) if init and any(b != 0.0 for b in init) else None
        self.table = self._t(_label_table(spec.labels))
        self._post_state()

    # the launches TreePlan shares with other kernels do not take this one
    def batch_launch_args(self, *args, **kw):
        return None

    def grouped_args(self, n_feat: int):
        return None

    def row_launcher(self, X, score, valid):
        return None

    def launch(self, X, score, valid, stream=None, probs=None, row_valid=None, splits: Optional[int] = None,
               score2=None, valid2=None) -> None:
        import ctypes

        from ..ops._lib import ClassTreeArgs, check, ptr, stream_handle

        n = X.shape[0]
        if X.shape[1] == 0:  # feature-less trees: the kernel still stages one column (TreePlan.launch)
            import torch

            X = torch.zeros((n, 1), dtype=torch.float32, device=X.device)
        if X.shape[1] < max(1, self.n_features):
            raise ValueError(f"expected [rows, {self.n_features}] input, got {tuple(X.shape)}")
        a = ClassTreeArgs()
        a.X, a.n_rows, a.n_feat, a.ldx, a.n_stage = X.data_ptr(), n, X.shape[1], X.stride(0), self.n_stage
        a.prep, a.row_valid_in, a.feat_map = ptr(self.prep), ptr(row_valid), ptr(self.feat_map)
        a.nodes, a.roots, a.leaves, a.acc_init = ptr(self.blob), ptr(self.roots), ptr(self.leaves), ptr(self.acc_init)
        a.n_trees, a.C, a.Cp, a.dense = self.n_trees, self.C, self.Cp, self.dense
        a.epi = _epilogue(table=self.table, write_probs=probs is not None, **self.epi_args)
        a.epi.score2, a.epi.valid2 = _addr(score2), _addr(valid2)
        a.score, a.valid, a.probs = _addr(score), _addr(valid), ptr(probs)
        check(self.lib.pmml_tree_classes_launch(stream_handle(stream), ctypes.byref(a)),
              f"class-tile tree kernel ({self.C} classes, depth {self.depth})")
