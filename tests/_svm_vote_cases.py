"""Documents and an independent float64 reference for the class outputs of SVM classifiers.

Two sources of documents, all with linear kernels on integer data (every decision value is an exact
small integer, many of them exactly on the threshold 0, so device and oracle count the same votes):

* ``_exact.svm_probe`` / ``_exact.svm_matrix`` by import (``probe_case``): every classification entry of
  ``_exact.SVM_CASES``, with Output fields added. On their 513 rows 97.3 % are valid and the winner is a
  tie in vote counts on 14 - 43 % of the rows of every multi-class case.
* ``VoteCase`` for what ``SvmProbe`` cannot write: a string target (the scoring plan answers
  ``EmptyScore``, the output plan decodes the labels), ``OneAgainstAll`` machines without an alternate
  (rows on which no machine votes), ``maxWins``, 8 machines over 16 categories (the fused kernels'
  limits together), 128 machines over 256 categories (the wide kernel's largest LDS request) and one
  case past the fused limits for the GEMM plan.

``reference`` computes votes, winner, validity and float64 shares from the dense decision values and
knows nothing of ``SvmEvaluator.finish``: machine m votes ``tgt`` when ``D_m < 0`` (``D_m >= 0`` under
``maxWins``), else ``alt`` if it has one; the winner is the first category with the most votes; a share
is ``votes_c / total`` (0/0 = NaN on a valid row without votes); a row with a missing field is invalid
and holds NaN.
"""

from __future__ import annotations

import io
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from _exact import SVM_CASES, assert_exact, svm_matrix, svm_probe
from _knn_vote_cases import bits, top_k, with_outputs  # noqa: F401  (re-exported for the tests)

F32 = np.float32


class VoteCase:
    """``machines``: ``(target category, alternate category or None)`` per machine; ``declared``: the
    target's ``<Value>`` list (the model's categories are these, then any other a machine names)."""

    def __init__(self, name: str, n_features: int, n_sv: int, machines: Sequence[Tuple[str, Optional[str]]],
                 declared: Sequence[str], seed: int, method: str = "OneAgainstOne", max_wins: bool = False,
                 target_type: str = "string", impl: str = "auto", plan: str = "SvmPlan"):
        rng = np.random.default_rng(seed)
        self.name, self.F, self.n_sv, self.method, self.max_wins = name, n_features, n_sv, method, max_wins
        self.target_type, self.impl, self.plan = target_type, impl, plan
        self.declared = list(declared)
        self.categories = list(declared)
        for t, a in machines:
            for c in (t, a):
                if c is not None and c not in self.categories:
                    self.categories.append(c)
        self.S = rng.integers(-2, 3, size=(n_sv, n_features)).astype(np.float64)
        self.machines = []
        M = len(machines)
        self.A = np.zeros((n_sv, M))
        self.b = np.zeros(M)
        for m, (t, a) in enumerate(machines):
            ids = np.sort(rng.choice(n_sv, size=min(n_sv, 5), replace=False))
            coef = (rng.integers(1, 4, size=len(ids)) * rng.choice([-1, 1], size=len(ids))).astype(np.float64)
            b0 = float(coef[0] * rng.integers(-1, 2))  # decision values land exactly on the threshold 0
            self.machines.append((ids, coef, b0, t, a))
            self.A[ids, m] = coef
            self.b[m] = b0

    @property
    def n_classes(self) -> int:
        return len(self.categories)

    def head(self) -> str:
        """The document up to its model element: header and data dictionary."""
        o = io.StringIO()
        o.write('<?xml version="1.0" encoding="UTF-8"?>\n<PMML xmlns="http://www.dmg.org/PMML-4_4" version="4.4">\n'
                f' <Header description="exact SVM votes {self.name}"/>\n'
                f' <DataDictionary numberOfFields="{self.F + 1}">\n')
        for j in range(self.F):
            o.write(f'  <DataField name="f{j}" optype="continuous" dataType="float"/>\n')
        o.write(f'  <DataField name="y" optype="categorical" dataType="{self.target_type}">'
                + "".join(f'<Value value="{v}"/>' for v in self.declared) + '</DataField>\n </DataDictionary>\n')
        return o.getvalue()

    def pmml(self, outputs: Sequence[str] = ()) -> str:
        return self.head() + self.model_xml(outputs) + '</PMML>\n'

    def model_xml(self, outputs: Sequence[str] = ()) -> str:
        """The ``SupportVectorMachineModel`` element alone (a segment of ``segmented_document``)."""
        o = io.StringIO()
        F = self.F
        mw = ' maxWins="true"' if self.max_wins else ""
        o.write(f' <SupportVectorMachineModel functionName="classification" svmRepresentation="SupportVectors" '
                f'classificationMethod="{self.method}"{mw}>\n'
                '  <MiningSchema>\n   <MiningField name="y" usageType="predicted"/>\n')
        for j in range(F):
            o.write(f'   <MiningField name="f{j}"/>\n')
        o.write('  </MiningSchema>\n')
        if outputs:
            o.write('  <Output>' + "".join(outputs) + '</Output>\n')
        o.write('  <LinearKernelType/>\n'
                f'  <VectorDictionary numberOfVectors="{self.n_sv}">\n   <VectorFields numberOfFields="{F}">')
        o.write("".join(f'<FieldRef field="f{j}"/>' for j in range(F)) + '</VectorFields>\n')
        for i in range(self.n_sv):
            o.write(f'   <VectorInstance id="sv{i}"><Array n="{F}" type="real">'
                    + " ".join(str(int(v)) for v in self.S[i]) + '</Array></VectorInstance>\n')
        o.write('  </VectorDictionary>\n')
        for ids, coef, b0, t, a in self.machines:
            alt = f' alternateTargetCategory="{a}"' if a is not None else ""
            o.write(f'  <SupportVectorMachine targetCategory="{t}"{alt}>\n'
                    f'   <SupportVectors numberOfSupportVectors="{len(ids)}">')
            o.write("".join(f'<SupportVector vectorId="sv{i}"/>' for i in ids) + '</SupportVectors>\n')
            o.write(f'   <Coefficients numberOfCoefficients="{len(ids)}" absoluteValue="{int(b0)}">')
            o.write("".join(f'<Coefficient value="{int(c)}"/>' for c in coef))
            o.write('</Coefficients>\n  </SupportVectorMachine>\n')
        o.write(' </SupportVectorMachineModel>\n')
        return o.getvalue()

    def votes(self, X: np.ndarray):
        """``(votes int64 [rows, C], ok bool [rows], D [rows, machines])``."""
        X = np.asarray(X, np.float64)
        ok = ~np.isnan(X).any(axis=1)
        G = np.nan_to_num(X) @ self.S.T
        D = G @ self.A + self.b
        assert_exact([G, D, np.abs(G) @ np.abs(self.A)])
        v = np.zeros((len(X), self.n_classes), dtype=np.int64)
        for m, (_, _, _, t, a) in enumerate(self.machines):
            first = D[:, m] >= 0 if self.max_wins else D[:, m] < 0
            v[first, self.categories.index(t)] += 1
            if a is not None:
                v[~first, self.categories.index(a)] += 1
        return v, ok, D


class ProbeCase:
    """An ``_exact.SVM_CASES`` classification entry: ``SvmProbe`` with Output fields added."""

    def __init__(self, name: str, kernel: str = "linear"):
        self.name = name
        self.probe, self.plan = svm_probe(name, kernel=kernel)
        self.F, self.n_sv = self.probe.F, self.probe.n_sv
        self.categories = [str(c) for c in range(self.probe.n_classes)]
        self.declared = list(self.categories)
        self.target_type, self.max_wins = "integer", False
        self.impl = "wide" if self.plan == "SvmWidePlan" else "fused"

    @property
    def n_classes(self) -> int:
        return len(self.categories)

    def pmml(self, outputs: Sequence[str] = ()) -> str:
        return with_outputs(self.probe.pmml(), outputs) if outputs else self.probe.pmml()

    def votes(self, X: np.ndarray):
        _, ok, D = self.probe.reference(X)
        v = np.zeros((len(X), self.n_classes), dtype=np.int64)
        for m, (_, _, _, a, b) in enumerate(self.probe.machines):
            first = D[:, m] < 0
            v[first, a] += 1
            v[~first, b] += 1
        return v, ok, D


def reference(c, X: np.ndarray):
    """``(label float64 (class index, NaN: no prediction), valid, shares float64 [rows, C], total)``."""
    v, ok, _ = c.votes(X)
    total = v.sum(axis=1)
    best = v.max(axis=1, keepdims=True)
    lab = np.argmax(v == best, axis=1).astype(np.float64)  # the first category with the most votes
    with np.errstate(invalid="ignore", divide="ignore"):
        shares = v.astype(np.float64) / total[:, None].astype(np.float64)
    return np.where(ok, lab, np.nan), ok, np.where(ok[:, None], shares, np.nan), total


def rows(c, n: int, seed: int = 5) -> np.ndarray:
    return svm_matrix(n, c.F, seed=seed)


def class_outputs(c, top: int = 6) -> List[str]:
    """``lab`` / ``shown`` / ``pwin`` / ``p_<class>`` of the first and the last classes / ``p_nobody`` (a
    class unknown to the model)."""
    cat, tt = "categorical", c.target_type
    out = [f'<OutputField name="lab" feature="predictedValue" optype="{cat}" dataType="{tt}"/>',
           f'<OutputField name="shown" feature="predictedDisplayValue" optype="{cat}" dataType="{tt}"/>',
           '<OutputField name="pwin" feature="probability" optype="continuous" dataType="double"/>']
    names = list(dict.fromkeys(c.categories[:top] + c.categories[-2:]))
    out += [f'<OutputField name="p_{x}" feature="probability" value="{x}" optype="continuous" dataType="double"/>'
            for x in names]
    out.append('<OutputField name="p_nobody" feature="probability" value="nobody" optype="continuous" '
               'dataType="double"/>')
    return out


def expected_columns(c, schema, X: np.ndarray) -> Dict[str, np.ndarray]:
    """The float64 Output columns of ``class_outputs(c)`` from the reference alone (``schema.lookup`` encodes
    the labels)."""
    lab, ok, shares, _ = reference(c, X)
    idx = np.where(ok, np.nan_to_num(lab), 0).astype(np.int64)
    cols = {}
    for name in ("lab", "shown"):
        codes = np.array([schema.lookup(name, x) for x in c.categories], dtype=np.float64)
        cols[name] = np.where(ok, codes[idx], np.nan)
    cols["pwin"] = np.where(ok, shares[np.arange(len(X)), idx], np.nan)
    for j, x in enumerate(c.categories):
        cols[f"p_{x}"] = shares[:, j]
    cols["p_nobody"] = np.zeros(len(X))  # a constant column: 0 on a row without a prediction too
    return cols


def _ovo(cats: Sequence[str]) -> List[Tuple[str, str]]:
    return [(a, b) for i, a in enumerate(cats) for b in cats[i + 1:]]


def _vote_cases() -> Dict[str, VoteCase]:
    L = [f"c{i:03d}" for i in range(256)]
    cases = [
        # a string target; "late" is declared by no <Value>: the model's last category
        VoteCase("str-ovo3", 9, 12, _ovo(["ant", "bee", "cat"]) + [("late", "ant")], ["ant", "bee", "cat"], seed=1),
        # OneAgainstAll without alternates on the matrix-core kernel: rows on which nobody votes
        VoteCase("oaa-noalt", 8, 33, [(x, None) for x in ("p", "q", "r", "s")], ["p", "q", "r", "s"], seed=2,
                 method="OneAgainstAll"),
        VoteCase("oaa-noalt-wide", 16, 33, [(x, None) for x in L[:3]], L[:5], seed=7, method="OneAgainstAll",
                 impl="wide", plan="SvmWidePlan"),
        VoteCase("maxwins", 9, 33, _ovo(["0", "1", "2", "3"]), ["0", "1", "2", "3"], seed=3, max_wins=True,
                 target_type="integer"),
        # the fused kernels' limits together: 8 machines, 16 categories
        VoteCase("m8c16", 8, 40, [(L[2 * m], L[2 * m + 1]) for m in range(8)], L[:16], seed=4),
        VoteCase("m8c16-valu", 8, 16, [(L[2 * m + 1], L[2 * m]) for m in range(8)], L[:16], seed=8),
        # the wide kernel's largest LDS request: 128 machines over 256 categories (CW = 128)
        VoteCase("m128c256", 16, 64, [(L[2 * m], L[2 * m + 1]) for m in range(128)], L, seed=5, impl="wide",
                 plan="SvmWidePlan"),
        # past the fused limits (9 machines, 18 categories) on the GEMM plan
        VoteCase("gemm-m9c18", 10, 20, [(L[2 * m], L[2 * m + 1]) for m in range(9)], L[:18], seed=6, impl="gemm",
                 plan="SvmGemmPlan"),
    ]
    return {c.name: c for c in cases}


VOTE_CASES = _vote_cases()
NO_VOTE_CASES = ("oaa-noalt", "oaa-noalt-wide")  # hold valid rows on which no machine votes


def segmented_document(method: str) -> str:
    """A classification MiningModel over three SVM segments (integer target, classes 0..3): the first
    behind ``f0 > 0``, the others always. Segment aggregation reads ``ModelResult.probs``, which an SVM
    leaves None."""
    cats = ["0", "1", "2", "3"]
    segs = [VoteCase(f"seg{i}", 9, 12, _ovo(cats), cats, seed=20 + i, target_type="integer") for i in range(3)]
    preds = ['<SimplePredicate field="f0" operator="greaterThan" value="0"/>', "<True/>", "<True/>"]
    o = io.StringIO()
    o.write(segs[0].head() + ' <MiningModel functionName="classification">\n'
            '  <MiningSchema>\n   <MiningField name="y" usageType="predicted"/>\n'
            + "".join(f'   <MiningField name="f{j}"/>\n' for j in range(9)) + '  </MiningSchema>\n'
            f'  <Segmentation multipleModelMethod="{method}">\n')
    for i, (seg, pred) in enumerate(zip(segs, preds)):
        o.write(f'   <Segment id="{i + 1}" weight="{i + 1}">{pred}\n{seg.model_xml()}   </Segment>\n')
    o.write('  </Segmentation>\n </MiningModel>\n</PMML>\n')
    return o.getvalue()


SEGMENT_METHODS = ("majorityVote", "weightedMajorityVote", "selectFirst", "average")
SEGMENT_ROWS = 64
PROBE_NAMES = [n for n, spec in SVM_CASES.items() if spec[2] >= 2]


def case(name: str):
    return VOTE_CASES[name] if name in VOTE_CASES else ProbeCase(name)


ALL_NAMES = PROBE_NAMES + sorted(VOTE_CASES)


def decided_rows(probe, X: np.ndarray) -> np.ndarray:
    """Rows of a polynomial / RBF / sigmoid ``SvmProbe`` on which every machine's float64 decision value
    is further from its threshold 0 than twice the bound ``tests/test_gpu_exact.py`` pins for the device's
    decision values (``SVM_ULP_CONSTANT * 2^-24 * T``, T: ``SvmProbe.kernel_terms``): there an fp32
    evaluation within that bound casts the oracle's votes."""
    from _exact import SVM_ULP_CONSTANT

    D, T = probe.kernel_terms(X)
    return (np.abs(D) > 2.0 * SVM_ULP_CONSTANT * 2.0 ** -24 * T).all(axis=1)
