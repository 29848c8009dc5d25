"""``OutputPlan``: a model's ``<Output>`` fields (and top-k classes) for whole batches on the device.

The scoring plans return one double per record — the target value as the reference extracts it.
An :class:`OutputPlan` owns a *second* plan of the same model, switched to index mode (its
epilogue's label table off: the score is the class / cluster index), and lowers
``compiled.model.output`` into the column program of ``ops/csrc/outputs.hip``: one kernel turns
the raw per-row results (index, validity, class probabilities, affinity) into the output columns
and into the reference score the scoring plan would have written. ``transformedValue`` /
``decision`` outputs that carry an expression run afterwards as one ``derive.hip`` program over
``[the input columns they read | the kernel's columns]``.

Columns reproduce ``models/base.py::_output_column`` (string-typed outputs as their ``schema.lookup``
encodings). What a family cannot provide raises :class:`NotLowerable` naming the output field.

With ``reason_codes=True`` the ``reasonCode`` fields (rank 1 … 8) of a Scorecard are columns too:
``ops/csrc/reasons.hip`` ranks the codes of every row on the plan's stream, after ``outputs_kernel``
has written ``valid``, from the matrix the scorecard's tree kernel read (``runtime/reasons.py``), and
writes them straight into their columns of the output matrix. Without the switch such a field is
refused by name, as is ``rank > 1`` of every other feature.

With ``entity_ranks=True`` the ranked-entity fields of a model whose plan is a ``ClusterPlan`` or a
``KnnPlan`` are columns as well: ``entityId`` / ``clusterId`` / affinity of rank 1 … 32, the affinity
of a named cluster, the neighbours' ids and distances of a k-NN model (``runtime/entities.py``).
``ops/csrc/entities.hip`` ranks the entities of every row on the plan's stream after
``outputs_kernel``, from the rows and the tensors the plan's own kernel read, and writes its columns
straight into the output matrix. Class outputs of a k-NN classifier stay refused by name unless
``knn_classes=True``.

With ``knn_classes=True`` the class outputs of a k-NN classifier are columns too. For ``k > 1`` the
inner ``KnnPlan`` runs in index mode (``class_table = None``): the class-output instantiation of
``ops/csrc/knn.hip`` writes the winning class index and the ``[rows, C]`` vote shares
(``votes_c / Σ votes``; NaN in a row without a prediction), and ``predictedValue`` /
``predictedDisplayValue``, ``probability`` (winner, named class) and ``top_k`` are the ordinary
column ops over them. A 1-NN classifier stays on ``ClusterPlan`` (the raw result is the nearest
instance's index): its ``probability`` columns are tables over the instances holding 1 / 0;
``top_k`` needs the matrix and is refused for it. More than 256 classes are refused naming the first
class field. Entity fields of the same document still go to the entity kernel (``entity_ranks=True``)
or are refused by name.

With ``svm_classes=True`` the class outputs of an SVM classifier are columns as well. The inner
``SvmPlan`` / ``SvmWidePlan`` / ``SvmGemmPlan`` runs in index mode (``table = None``): the class-output
instantiations of ``ops/csrc/svm.hip`` (the tensor program of ``SvmGemmPlan``) write the winning class
index and the ``[rows, C]`` vote shares (``votes_c / Σ votes``; NaN in a row without a prediction and
in a valid row on which no machine voted), and the ordinary column ops read them. More than 256
classes are refused naming the first class field. Without the switch every class output of an SVM is
refused by name.

With ``association_rules=True`` an AssociationModel has an output plan at all: it has no target field,
so there is no inner scoring plan (without the switch ``compile_plan`` refuses it). ``launch`` fills
``score`` with NaN and ``valid`` with 0, and ``ops/csrc/rules.hip`` ranks the matching rules of every
row from the raw rows and the document's ``FieldPrep`` (``runtime/rules.py``), writing the
``ruleValue`` / ``entityId`` columns straight into the output matrix. Fields the base oracle answers
with NaN are ``OP_NAN`` columns; an expression beside them and ``top_k`` are refused by name. A row
that fails the preparation holds NaN in every rule column, as on the host.

Known difference from the host path: a row that fails the MiningField preparation has NaN in every
column on the host; on the device such a row is a row without a prediction, so a constant column
(the probability of an undeclared class) and an expression that maps missing values keep their value.
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np

from ..models.base import ModelEvaluator, class_probabilities
from ..ops import outputs as K
from .plans import DevicePlan, NotLowerable, build_field_prep, compile_plan

_NAN_FEATURES = ("warning", "reasonCode", "ruleValue", "residual", "standardError", "confidence")


def _base(plan):
    while getattr(plan, "inner", None) is not None:
        plan = plan.inner
    return plan


def oracle_top_k(probs: np.ndarray, valid: np.ndarray, k: int):
    """Top-k of the oracle's ``ModelResult.probs`` under the kernel's rule: stable descending sort
    (ties to the lower class), NaN never selected, NaN / -1 past the non-NaN classes and on invalid
    rows. Returns ``(index int64 [n, k], probability float64 [n, k])``."""
    n = len(valid)
    idx = np.full((n, k), -1, dtype=np.int64)
    pr = np.full((n, k), np.nan)
    if probs is None or k == 0:
        return idx, pr
    P = np.asarray(probs, dtype=np.float64)
    # descending by value, NaN strictly last (behind a -inf probability too), stable in the class index
    miss = np.isnan(P)
    order = np.lexsort((np.where(miss, 0.0, -P), miss), axis=1)[:, :k]
    top = np.take_along_axis(P, order, axis=1)
    keep = ~np.isnan(top) & np.asarray(valid, dtype=bool)[:, None]
    w = order.shape[1]
    idx[:, :w] = np.where(keep, order, -1)
    pr[:, :w] = np.where(keep, top, np.nan)
    return idx, pr


class OutputPlan(DevicePlan):
    kind = "outputs"
    supports_direct = False

    def __init__(self, compiled, device, top_k: int = 0, reason_codes: bool = False, entity_ranks: bool = False,
                 knn_classes: bool = False, svm_classes: bool = False, association_rules: bool = False, **opts):
        super().__init__(compiled, device)
        from ..models.association import AssociationEvaluator
        from ..models.scorecard import ScorecardEvaluator
        from .nn_plans import GemmMlpPlan, MlpPlan, SvmGemmPlan, SvmPlan, SvmWidePlan
        from .plans import ClusterPlan, KnnPlan, LinearPlan, TreePlan
        from .segmented import SegmentedPlan, _index_outputs, probs_width

        top_k = int(top_k)
        if not 0 <= top_k <= K.MAX_TOP_K:
            raise ValueError(f"top_k must be in [0, {K.MAX_TOP_K}], got {top_k}")
        self.top_k = top_k
        ev = compiled.evaluator
        self.rules = None  # the packed association rules (ops.rules.RuleTables) when the rule kernel runs
        self._association = False
        if bool(association_rules) and isinstance(ev, AssociationEvaluator):
            self._lower_association(compiled, ev)  # no target, no inner scoring plan: the rule kernel alone
            return
        # reasonCode fields of a scorecard rank on the device (ops/csrc/reasons.hip); off: refused by name
        self._rank_reasons = bool(reason_codes) and isinstance(ev, ScorecardEvaluator)
        self.reasons = None  # the packed scorecard (ops.reasons.ReasonTables) when a reason kernel runs
        self._reason_prep = None
        if self._rank_reasons and ev.scorecard.use_reason_codes:
            from .reasons import check_baselines

            asked = [of for of in compiled.model.output if of.feature == "reasonCode"]
            if asked:  # the oracle raises on every batch, the probe below included
                check_baselines(ev.scorecard, asked[0])
        # what the oracle's result holds for this model: one all-missing row through it
        probe = ev.evaluate(compiled.columns(np.full((1, compiled.n_features), np.nan)))
        self.result_kind = probe.kind
        self.inner = compile_plan(compiled, device, **opts)  # this plan's own: the cached scoring plan stays as is
        base = _base(self.inner)
        # ranked-entity fields of the distance families rank on the device (ops/csrc/entities.hip)
        self._rank_entities = bool(entity_ranks) and isinstance(base, (ClusterPlan, KnnPlan))
        self.entities = None  # ops.entities.EntityTables when an entity kernel runs
        classes = probe.kind in ("classification", "clustering")
        labels: Optional[List[str]] = None
        C = None
        self._affinity = False
        # class outputs of a k-NN classifier: the vote kernel's index mode (k > 1), tables over the
        # instances (k = 1 on ClusterPlan)
        knn_votes = bool(knn_classes) and getattr(ev, "knn", None) is not None and probe.kind == "classification"
        self._knn_one = knn_votes and isinstance(base, ClusterPlan)
        self._knn_index = False
        if knn_votes and isinstance(base, KnnPlan) and base.labels is not None:
            if len(base.labels) > K.MAX_CLASSES:
                asked = [of for of in compiled.model.output
                         if of.feature in ("predictedValue", "predictedDisplayValue", "probability")]
                if asked:
                    raise NotLowerable(f"output {asked[0].name!r}: {len(base.labels)} classes > {K.MAX_CLASSES}")
                if top_k:
                    raise NotLowerable(f"top_k: {len(base.labels)} classes > {K.MAX_CLASSES}")
            else:
                labels = list(base.labels)
                C = len(labels)
                self._knn_index = True
        # class outputs of an SVM classifier: the vote kernels' index mode (table = None) and their shares
        self._svm_index = False
        if bool(svm_classes) and isinstance(base, (SvmPlan, SvmWidePlan, SvmGemmPlan)) \
                and probe.kind == "classification":
            if len(ev.categories) > K.MAX_CLASSES:  # only reachable on SvmGemmPlan
                asked = [of for of in compiled.model.output
                         if of.feature in ("predictedValue", "predictedDisplayValue", "probability")]
                if asked:
                    raise NotLowerable(f"output {asked[0].name!r}: {len(ev.categories)} classes > {K.MAX_CLASSES}")
                if top_k:
                    raise NotLowerable(f"top_k: {len(ev.categories)} classes > {K.MAX_CLASSES}")
            else:
                labels = list(ev.categories)
                C = len(labels)
                self._svm_index = True
        if isinstance(base, ClusterPlan):
            labels = list(ev.entity_ids)
        elif isinstance(base, (LinearPlan, TreePlan)):
            if classes:
                own = base.labels if isinstance(base, TreePlan) else base.compiled.evaluator.categories
                labels = list(own) if own is not None else None
                C = probs_width(self.inner)
        elif isinstance(base, MlpPlan) and not isinstance(base, GemmMlpPlan):  # the fused and the wide kernels
            if classes:
                labels = list(base.labels)
                C = len(labels)
        elif isinstance(base, SegmentedPlan):
            if classes:
                labels = list(base.categories)
        self._no_index = None
        if classes and labels is None:  # every class / entity output of such a model is refused by name
            self._no_index = f"{type(base).__name__} has no index mode (class / entity outputs are host-only)"
        elif classes and any(x is None for x in labels):
            raise NotLowerable("outputs: the plan does not know its class labels")
        self.labels = labels
        self.label_table = None
        if labels is not None:
            own = base.class_table if self._knn_index else getattr(base, "table", None)
            if own is None or int(own.numel()) != len(labels):
                raise NotLowerable("outputs: the plan's label table does not match its classes")
            table = own.detach().cpu().numpy().astype(np.float32)
            self.label_table = self._t(np.append(table, np.float32(np.nan)))
            self.label_values = table
            if self._knn_index:
                base.class_table = None  # the vote kernel's index mode
            elif isinstance(base, (ClusterPlan, SegmentedPlan)):
                # their kernels always read the table: the identity table is the index mode
                base.table = self._t(np.arange(len(labels), dtype=np.float32))
                if isinstance(base, SegmentedPlan):
                    base._post_build()
            else:
                _index_outputs(self.inner)
        if C is not None and C != len(labels):
            C = None  # the plan's probability columns are not its classes
        if C is not None and C > K.MAX_CLASSES:
            raise NotLowerable(f"outputs: {C} classes > {K.MAX_CLASSES}")
        # the oracle's class order (probabilities, top-k) against the plan's index order
        self.categories = list(probe.categories) if probe.categories is not None else None
        self._lower(compiled, ev, probe, base, C, isinstance(base, ClusterPlan))

    # ------------------------------------------------------------------ lowering
    def _lower(self, compiled, ev, probe, base, C: Optional[int], cluster: bool) -> None:
        from ..ops import reasons as R
        from .derive import _expr_fields
        from .entities import is_entity_field, lower_entities
        from .segmented import expression_program

        schema = compiled.schema
        labels = self.labels
        prog: List[tuple] = []
        tables: List[float] = []
        self.names = [of.name for of in compiled.model.output]
        self.kernel_names: List[str] = []  # the kernel's columns, in order
        exprs = []
        reason_fields = []  # (Output field, its column of the matrix): written by the reason kernel
        entity_fields = []  # likewise, written by the entity kernel
        # the vote kernels' index mode always writes its shares
        need_probs = self.top_k > 0 or self._knn_index or self._svm_index
        need_aff = False
        custom = type(ev)._output_column is not ModelEvaluator._output_column

        def table(values) -> int:
            off = len(tables)
            tables.extend(float(v) for v in values)
            return off

        def no(of, why: str):
            return NotLowerable(f"output {of.name!r}: {why}")

        for of in compiled.model.output:
            feat = of.feature
            if self._rank_entities and is_entity_field(of, ev):
                entity_fields.append((of, self.names.index(of.name)))
                continue
            if self._no_index:
                raise no(of, self._no_index)
            if self._rank_reasons and feat == "reasonCode":
                if int(of.rank) > R.MAX_RANK:
                    raise no(of, f"reason code rank {of.rank} > {R.MAX_RANK}")
                if ev.scorecard.use_reason_codes:
                    reason_fields.append((of, self.names.index(of.name)))
                    continue
                prog.append((K.OP_NAN, 0, 0))  # useReasonCodes="false": no codes, as the oracle
                self.kernel_names.append(of.name)
                continue
            if int(getattr(of, "rank", 1) or 1) > 1:
                raise no(of, f"rank {of.rank} > 1 is not evaluated")
            if custom and feat in ("reasonCode", "ruleValue", "entityId"):
                raise no(of, f"{feat} of a {type(ev).__name__} is host-only")
            if feat in ("transformedValue", "decision") and of.expression is not None:
                exprs.append((of, len(self.kernel_names)))
                continue
            if feat in ("predictedValue", "predictedDisplayValue"):
                if probe.kind == "regression" and labels is not None:
                    # a 1-NN regression on ClusterPlan: the raw result is the nearest instance's index
                    col = (K.OP_TABLE, len(labels), table([float(v) for v in self.label_values] + [np.nan]))
                elif probe.kind == "regression":
                    col = (K.OP_VALUE, 0, 0)
                elif labels is not None:
                    col = (K.OP_TABLE, len(labels), table([schema.lookup(of.name, x) for x in labels] + [np.nan]))
                else:
                    col = (K.OP_NAN, 0, 0)
            elif feat == "probability":
                if class_probabilities(probe) is None or probe.categories is None:
                    raise no(of, "the model has no probabilities")
                if self._knn_one:
                    # the nearest instance casts the only vote: 1 for its class, 0 for every other
                    if of.value is None:
                        col = (K.OP_TABLE, len(labels), table([1.0] * len(labels) + [np.nan]))
                    elif of.value not in probe.categories:
                        col = (K.OP_CONST, 0, table([0.0]))
                    else:
                        col = (K.OP_TABLE, len(labels), table([float(x == of.value) for x in labels] + [np.nan]))
                    prog.append(col)
                    self.kernel_names.append(of.name)
                    continue
                if C is None:
                    raise no(of, f"{type(base).__name__} does not expose probabilities")
                if of.value is None:
                    col = (K.OP_PROB_WINNER, 0, 0)
                elif of.value not in probe.categories:
                    col = (K.OP_CONST, 0, table([0.0]))
                elif of.value not in labels:
                    raise no(of, f"class {of.value!r} is unknown to the device plan")
                else:
                    col = (K.OP_PROB, labels.index(of.value), 0)
                need_probs = True
            elif feat in ("entityId", "clusterId"):
                if probe.kind != "clustering" or not cluster:
                    raise no(of, f"{feat} (entity ranks) of this model is host-only")
                if feat == "clusterId":
                    col = (K.OP_TABLE, len(labels), table([i + 1.0 for i in range(len(labels))] + [np.nan]))
                else:
                    col = (K.OP_TABLE, len(labels), table([schema.lookup(of.name, x) for x in labels] + [np.nan]))
            elif feat in ("affinity", "clusterAffinity", "entityAffinity"):
                if probe.affinity is None or not cluster:
                    raise no(of, f"{feat} is not available on the device for this model")
                if of.value is not None and probe.entity_affinities is not None and probe.entity_ids is not None \
                        and of.value in probe.entity_ids:
                    raise no(of, f"{feat} of the named entity {of.value!r} is host-only")
                col = (K.OP_AFFINITY, 0, 0)
                need_aff = True
            elif feat == "transformedValue":
                col = (K.OP_VALUE, 0, 0) if probe.kind == "regression" else (K.OP_NAN, 0, 0)
            elif feat in _NAN_FEATURES:
                col = (K.OP_NAN, 0, 0)
            else:
                raise no(of, f"feature {feat!r} is not supported")
            prog.append(col)
            self.kernel_names.append(of.name)
        if self.top_k:
            if self._knn_one:
                raise NotLowerable("top_k: a 1-NN classifier runs on ClusterPlan, whose result is the nearest "
                                   "instance and not a vote matrix (top_k of k = 1 is host-only)")
            if C is None:
                raise NotLowerable(f"top_k: {type(base).__name__} does not expose class probabilities")
            if self.categories != labels:
                raise NotLowerable("top_k: the device plan orders the classes differently from the oracle")
            prog += [(K.OP_TOPK_INDEX, r, 0) for r in range(self.top_k)]
            prog += [(K.OP_TOPK_PROB, r, 0) for r in range(self.top_k)]
        self.n_named = len(self.kernel_names)  # kernel columns that are Output fields
        self.kernel_names += [f"__top_index_{r}" for r in range(self.top_k)] + \
                             [f"__top_probability_{r}" for r in range(self.top_k)]
        if not prog:
            prog.append((K.OP_NAN, 0, 0))  # the kernel writes at least one column
        self.n_col = len(prog)
        if self.n_col > K.MAX_COLUMNS:
            raise NotLowerable(f"outputs: {self.n_col} columns > {K.MAX_COLUMNS}")
        self.C = C if need_probs else None
        self._affinity = need_aff
        self.width = len(self.names) + 2 * self.top_k  # [Output fields | top-k indices | top-k probabilities]
        self.prog_np = np.array([(op, arg, off, 0) for op, arg, off in prog], dtype=np.int32).reshape(-1, 4)
        self.tables_np = np.array(tables or [0.0], dtype=np.float32)
        self.prog, self.tables = self._t(self.prog_np), self._t(self.tables_np)
        # where each kernel column / expression lands in the [rows, width] result
        pos = {n: i for i, n in enumerate(self.names)}
        self.kernel_dst = [pos[n] for n in self.kernel_names[: self.n_named]] + \
            list(range(len(self.names), self.width))
        self.direct_out = not exprs and self.kernel_dst == list(range(self.width)) and self.width == self.n_col
        if reason_fields:
            self._lower_reasons(compiled, ev, reason_fields)
        if entity_fields:
            if self.inner is not base:
                raise no(entity_fields[0][0], f"entity ranks need the rows {type(base).__name__} reads, "
                                              f"not those of a {type(self.inner).__name__}")
            self.entities = lower_entities(base, ev, schema, entity_fields, self.width)
        self.expr = None
        if exprs:
            used: List[str] = []
            for of, _ in exprs:
                _expr_fields(of.expression, lambda f: used.append(f) if f not in used else None)
            inputs = [f for f in used if f in compiled.active_fields and f not in self.names]
            for f in inputs:
                if build_field_prep(compiled, [f])[1]:
                    raise no(exprs[0][0], f"its expression reads {f!r}, whose MiningField preparation is not the identity")
            columns = inputs + self.kernel_names
            col_of = {f: i for i, f in enumerate(inputs)}
            items, shown = [], 0
            for of, n_before in exprs:  # outputs declared before an expression are visible to it
                reveal = {n: len(inputs) + i for i, n in enumerate(self.kernel_names[shown:n_before], start=shown)}
                shown = max(shown, n_before)
                items.append((of.name, of.expression, reveal))
            try:
                dp = expression_program(schema, columns, col_of, items, "output expression")
            except NotLowerable as e:
                raise NotLowerable(f"output expressions ({', '.join(of.name for of, _ in exprs)}): {e}") from e
            self.expr = (dp, self._t(dp.insns.view(np.int32).reshape(-1)), self._t(dp.pool), self._t(dp.out_cols),
                         [pos[of.name] for of, _ in exprs])
            self.expr_inputs = [compiled.active_fields.index(f) for f in inputs]
        self._dst = None

    def _lower_association(self, compiled, ev) -> None:
        """An AssociationModel under ``association_rules=True``: its ``ruleValue`` / ``entityId``
        fields go to the rule kernel (``runtime/rules.py``), the fields the base oracle answers with
        NaN stay ``OP_NAN`` columns of the column program, every other field is refused by name."""
        from .rules import RULE_FEATURES, lower_rules

        if self.top_k:
            raise NotLowerable("top_k: an AssociationModel has no classes")
        self._association = True
        self.result_kind = "association"
        self.inner = self.reasons = self.entities = self.expr = self._reason_prep = None
        self.labels = self.label_table = self.categories = self.C = self._no_index = None
        self._affinity = self._rank_reasons = self._rank_entities = False
        self._knn_one = self._knn_index = self._svm_index = False
        self.names = [of.name for of in compiled.model.output]
        self.width = len(self.names)
        self.kernel_names: List[str] = []
        rule_fields = []
        for j, of in enumerate(compiled.model.output):
            feat = of.feature
            if feat in RULE_FEATURES:
                rule_fields.append((of, j))
            elif feat in ("transformedValue", "decision") and of.expression is not None:
                raise NotLowerable(f"output {of.name!r}: an expression beside the rule columns of an "
                                   f"AssociationModel is host-only")
            elif feat in ("predictedValue", "predictedDisplayValue", "transformedValue") or feat in _NAN_FEATURES:
                self.kernel_names.append(of.name)  # no target, no result: NaN as the base oracle answers
            else:
                raise NotLowerable(f"output {of.name!r}: feature {feat!r} is not available for an AssociationModel")
        self.n_named = len(self.kernel_names)
        self.n_col = max(1, self.n_named)
        if self.n_col > K.MAX_COLUMNS:
            raise NotLowerable(f"outputs: {self.n_col} columns > {K.MAX_COLUMNS}")
        self.prog_np = np.array([(K.OP_NAN, 0, 0, 0)] * self.n_col, dtype=np.int32).reshape(-1, 4)
        self.tables_np = np.array([0.0], dtype=np.float32)
        self.prog, self.tables = self._t(self.prog_np), self._t(self.tables_np)
        self.kernel_dst = [self.names.index(n) for n in self.kernel_names]
        self.direct_out = False
        self._dst = None
        if rule_fields:
            self.rules = lower_rules(ev, compiled, rule_fields, self.width)

    def _launch_association(self, X, score, valid, st, outputs, score2, valid2) -> None:
        """No inner plan: every score is empty, the ``OP_NAN`` columns come from the column program
        over that empty result, the rule columns from ``rules.hip`` over the raw rows."""
        import torch

        from ..ops.rules import rules_launch

        n = int(X.shape[0])
        with torch.cuda.stream(st):
            raw_s = torch.full((n,), float("nan"), dtype=torch.float32, device=self.device)
            raw_v = torch.zeros(n, dtype=torch.uint8, device=self.device)
            if outputs is None:
                outputs = self.alloc_matrix(n)
            if self.kernel_dst:
                out = torch.empty((n, self.n_col), dtype=torch.float32, device=self.device)
                K.outputs_launch(raw_s, raw_v, out, self.prog, self.tables, stream=st)
                if self._dst is None:
                    self._dst = torch.tensor(self.kernel_dst, dtype=torch.int64, device=self.device)
                outputs.index_copy_(1, self._dst, out)
                out.record_stream(st)
            if self.rules is not None:
                rules_launch(X, outputs, self.rules, prep=self.prep, stream=st)
            for dst, src in ((score, raw_s), (valid, raw_v), (score2, raw_s), (valid2, raw_v)):
                if dst is not None:
                    dst.copy_(src)
            raw_s.record_stream(st)
            raw_v.record_stream(st)

    def _launch_association_host(self, X, score, valid, outputs, score2, valid2) -> None:
        """Lowering dry run of :meth:`_launch_association` through the kernels' numpy twins."""
        from ..ops.rules import rules_numpy

        Xn = np.asarray(X.numpy() if hasattr(X, "numpy") else X, dtype=np.float32)
        n = len(Xn)
        out, s, v = K.outputs_numpy(np.full(n, np.nan, dtype=np.float32), np.zeros(n, dtype=np.uint8), self.prog_np,
                                    self.tables_np)
        full = np.full((n, self.width), np.nan, dtype=np.float32)
        if self.kernel_dst:
            full[:, self.kernel_dst] = out[:, : len(self.kernel_dst)]
        if self.rules is not None:
            rules_numpy(Xn, full, self.rules, prep=self.prep.numpy() if self.prep is not None else None)
        for dst, src in ((score, s), (valid, v), (outputs, full), (score2, s), (valid2, v)):
            if dst is not None:
                (dst.numpy() if hasattr(dst, "numpy") else dst)[...] = src

    def _lower_reasons(self, compiled, ev, reason_fields) -> None:
        """The reason kernel reads the matrix the scorecard's general tree kernel reads: the raw
        rows with this plan's FieldPrep, or the tile the inner derive pass writes."""
        from .derive import DerivedPlan
        from .plans import TreePlan
        from .reasons import lower_reasons

        tree = self.inner.inner if isinstance(self.inner, DerivedPlan) else self.inner
        if not isinstance(tree, TreePlan) or tree.layout != "general":
            raise NotLowerable(f"output {reason_fields[0][0].name!r}: reason codes need the general tree plan, "
                               f"not {type(tree).__name__}")
        view = tree.compiled
        index = getattr(view, "field_index", None) or {f: i for i, f in enumerate(view.active_fields)}
        self.reasons = lower_reasons(ev.scorecard, compiled.schema, index, int(tree.n_features), reason_fields,
                                     self.width)
        self._reason_prep = tree.prep  # None behind a derive pass: the tile is prepared

    def _reason_matrix_host(self, Xn: np.ndarray) -> np.ndarray:
        """Dry run: the reason kernel's input for the raw fp32 rows ``Xn``."""
        from .derive import DerivedPlan, emulate

        if isinstance(self.inner, DerivedPlan):
            P, _ = self.compiled.prepare(Xn)
            return emulate(self.inner.program, P)
        return Xn

    # ------------------------------------------------------------------ execution
    def alloc_matrix(self, n: int):
        import torch

        return torch.empty((n, self.width), dtype=torch.float32, device=self.device)

    def launch(self, X, score, valid, stream=None, outputs=None, score2=None, valid2=None, **kw) -> None:
        """Score ``X`` (device ``[n, F]`` fp32) on ``stream``: ``score`` / ``valid`` take what the
        scoring plan writes, ``outputs`` (``[n, width]`` fp32, unit column stride) the Output
        fields in document order followed by the top-k indices and the top-k probabilities."""
        import torch

        n = int(X.shape[0])
        if n == 0:
            return
        if self.device.type != "cuda":
            self._launch_host(X, score, valid, outputs, score2, valid2)
            return
        from .segmented import run_expression_program

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if self._association:
            self._launch_association(X, score, valid, st, outputs, score2, valid2)
            return
        with torch.cuda.stream(st):
            raw_s = torch.empty(n, dtype=torch.float32, device=self.device)
            raw_v = torch.empty(n, dtype=torch.uint8, device=self.device)
            probs = torch.empty((n, self.C), dtype=torch.float32, device=self.device) if self.C else None
            aff = torch.empty(n, dtype=torch.float32, device=self.device) if self._affinity else None
            if outputs is None:
                outputs = self.alloc_matrix(n)
            out = outputs if self.direct_out else torch.empty((n, self.n_col), dtype=torch.float32, device=self.device)
            extra = {}
            if probs is not None:
                extra["probs"] = probs
            if aff is not None:
                extra["affinity"] = aff
            self.inner.launch(X, raw_s, raw_v, stream=st, **extra)
            K.outputs_launch(raw_s, raw_v, out, self.prog, self.tables, probs=probs, affinity=aff,
                             label_table=self.label_table, k=self.top_k, score_out=score, valid_out=valid, stream=st)
            if not self.direct_out and self.width:
                if self._dst is None:
                    self._dst = torch.tensor(self.kernel_dst, dtype=torch.int64, device=self.device)
                if self.kernel_dst:
                    outputs.index_copy_(1, self._dst, out[:, : len(self.kernel_dst)])
                if self.expr is not None:
                    Xa = torch.cat([X[:, self.expr_inputs], out], dim=1) if self.expr_inputs else out
                    res = run_expression_program(self.device, self.lib, self.expr, Xa.contiguous(), st)
                    for j, c in enumerate(self.expr[4]):
                        outputs[:, c] = res[:, j]
            if self.reasons is not None:
                from ..ops.reasons import reasons_launch
                from .derive import DerivedPlan

                # after outputs_kernel wrote ``valid``; a derive pass left its tile in this stream's buffer
                Xr = self.inner._buffers(st, n)[0] if isinstance(self.inner, DerivedPlan) else X
                reasons_launch(Xr, valid if valid is not None else raw_v, outputs, self.reasons,
                               prep=self._reason_prep, stream=st)
            if self.entities is not None:
                from ..ops.entities import entities_launch

                entities_launch(X, outputs, self.entities, prep=self.inner.prep, stream=st)
            if score2 is not None:
                score2.copy_(score)
                valid2.copy_(valid)
            for t in (raw_s, raw_v, probs, aff, out):
                if t is not None:
                    t.record_stream(st)

    def raw_from_oracle(self, X: np.ndarray):
        """The raw results the index-mode plan leaves for ``X``, from the float64 oracle (the dry-run
        stand-in for the model kernels): ``(score fp32, valid u8, probs fp32 or None, affinity or None)``."""
        c = self.compiled
        P, okp = c.prepare(np.asarray(X, dtype=np.float64))
        res, _ = c.evaluate_prepared(P)
        v = np.asarray(res.value, dtype=np.float64)
        valid = np.asarray(res.valid, dtype=bool) & okp & ~np.isnan(v)
        probs = None
        if self.labels is not None and self.result_kind == "regression":  # 1-NN on ClusterPlan: the index
            from ..models.base import ranked_entities

            v = np.where(valid, ranked_entities(res).index[:, 0], np.nan)
        if self.labels is not None and self.result_kind == "classification" and res.categories is not None \
                and list(res.categories) != self.labels:
            to_plan = np.array([self.labels.index(x) if x in self.labels else -1 for x in res.categories] + [-1])
            v = np.where(valid, to_plan[np.where(valid, v, len(res.categories)).astype(np.int64)], np.nan)
            if self.C:
                src = [list(res.categories).index(x) for x in self.labels]
                probs = np.asarray(class_probabilities(res))[:, src]
        elif self.C:
            probs = np.asarray(class_probabilities(res))
        aff = np.asarray(res.affinity, dtype=np.float32) if self._affinity else None
        return (np.where(valid, v, np.nan).astype(np.float32), valid.astype(np.uint8),
                None if probs is None else probs.astype(np.float32), aff)

    def _launch_host(self, X, score, valid, outputs, score2, valid2) -> None:
        """Lowering dry run: the oracle's raw results through the kernel's numpy twin and
        ``derive.emulate``."""
        from .derive import emulate

        if self._association:
            self._launch_association_host(X, score, valid, outputs, score2, valid2)
            return
        Xn = X.numpy() if hasattr(X, "numpy") else np.asarray(X)
        Xn = np.asarray(Xn, dtype=np.float32)
        raw_s, raw_v, probs, aff = self.raw_from_oracle(Xn)
        lt = self.label_table.numpy() if self.label_table is not None else None
        out, s, v = K.outputs_numpy(raw_s, raw_v, self.prog_np, self.tables_np, probs=probs, affinity=aff,
                                    label_table=lt, k=self.top_k)
        full = np.full((len(Xn), self.width), np.nan, dtype=np.float32)
        if self.kernel_dst:
            full[:, self.kernel_dst] = out[:, : len(self.kernel_dst)]
        if self.expr is not None:
            Xa = np.concatenate([Xn[:, self.expr_inputs], out], axis=1).astype(np.float64)
            res = emulate(self.expr[0], Xa)
            for j, c in enumerate(self.expr[4]):
                full[:, c] = res[:, j]
        if self.reasons is not None:
            from ..ops.reasons import reasons_numpy

            prep = self._reason_prep.numpy() if self._reason_prep is not None else None
            reasons_numpy(self._reason_matrix_host(Xn), v, full, self.reasons, prep=prep)
        if self.entities is not None:
            from ..ops.entities import entities_numpy

            prep = self.inner.prep.numpy() if self.inner.prep is not None else None
            entities_numpy(Xn, full, self.entities, prep=prep)
        for dst, src in ((score, s), (valid, v), (outputs, full), (score2, s), (valid2, v)):
            if dst is not None:
                (dst.numpy() if hasattr(dst, "numpy") else dst)[...] = src

    def score_outputs(self, X: Any, replace_nan: Optional[float] = None, stream=None, absent: Any = None):
        """Like :meth:`DevicePlan.score`: ``(score, valid bool, matrix [n, width])`` device tensors."""
        import torch

        if self.device.type != "cuda":
            Xn = np.asarray(X.numpy() if hasattr(X, "numpy") else X, dtype=np.float32)
            if replace_nan is not None:
                Xn = np.where(np.isnan(Xn) if absent is None else np.asarray(absent, dtype=bool),
                              np.float32(replace_nan), Xn)
            Xt = torch.from_numpy(np.ascontiguousarray(Xn))
        else:
            Xt = self._device_matrix(X, replace_nan, absent)
        score, valid = self.alloc_outputs(Xt.shape[0])
        matrix = self.alloc_matrix(Xt.shape[0])
        self.launch(Xt, score, valid, stream=stream, outputs=matrix)
        return score, valid.bool(), matrix

    def score_csr_outputs(self, batch, replace_nan: Optional[float] = None, stream=None):
        """:meth:`score_outputs` of a sparse batch, expanded on the device."""
        import torch

        from ..ops.sparse import MAX_WIDTH

        if self.device.type != "cuda" or self.n_features > MAX_WIDTH:
            return self.score_outputs(batch.X, replace_nan, stream=stream, absent=batch.absent)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            Xt = self._csr_device_matrix(batch, replace_nan, st)
            score, valid = self.alloc_outputs(len(batch))
            matrix = self.alloc_matrix(len(batch))
            self.launch(Xt, score, valid, stream=st, outputs=matrix)
            return score, valid.bool(), matrix


def oracle_outputs(compiled, X: np.ndarray, replace_nan: Optional[float] = None, absent: Optional[np.ndarray] = None,
                   top_k: int = 0):
    """The host path: ``(scores, valid, {name: float64 column}, ModelResult or None, row_ok)`` from
    one vectorised oracle pass; rows that fail preparation hold NaN in every column."""
    from ..models import result_scores

    P, ok = compiled.prepare(X, replace_nan, absent)
    n = P.shape[0]
    if not compiled.model.output and not top_k and not compiled.target_fields:
        return np.full(n, np.nan), np.zeros(n, dtype=bool), {}, None, ok
    res, outs = compiled.evaluate_prepared(P)
    if compiled.target_fields:
        s, v = result_scores(res)
        v = v & ok
        s = np.where(v, s, np.nan)
    else:
        s, v = np.full(n, np.nan), np.zeros(n, dtype=bool)
    cols: Dict[str, np.ndarray] = {k: np.where(ok, np.asarray(c, dtype=np.float64), np.nan) for k, c in outs.items()}
    return s, v, cols, res, ok


def host_batch_outputs(compiled, X: np.ndarray, replace_nan: Optional[float] = None,
                       absent: Optional[np.ndarray] = None, top_k: int = 0):
    """``(scores, valid, BatchOutputs)`` on the host: :func:`oracle_outputs` as the float64 matrix
    of the model's Output fields in document order, plus the top-k of ``ModelResult.probs``."""
    from ..api.batch import BatchOutputs

    top_k = int(top_k)
    if not 0 <= top_k <= K.MAX_TOP_K:
        raise ValueError(f"top_k must be in [0, {K.MAX_TOP_K}], got {top_k}")
    s, v, cols, res, ok = oracle_outputs(compiled, X, replace_nan, absent, top_k)
    names = [of.name for of in compiled.model.output]
    n = len(s)
    matrix = np.stack([cols[k] for k in names], axis=1) if names else np.empty((n, 0))
    ti = tp = cats = None
    if res is not None and res.categories is not None:
        cats = list(res.categories)
    if top_k:
        probs = class_probabilities(res) if res is not None else None
        if probs is None:
            raise NotLowerable("top_k: the model has no class probabilities")
        ti, tp = oracle_top_k(probs, np.asarray(res.valid, dtype=bool) & ok, top_k)
    return s, v, BatchOutputs(names, matrix, compiled.schema, cats, ti, tp)


__all__ = ["OutputPlan", "host_batch_outputs", "oracle_outputs", "oracle_top_k"]
