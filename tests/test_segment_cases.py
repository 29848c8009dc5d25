"""The prescribed segment results of ``tests/_segment_cases.py`` are exact, populated and sensitive
(CPU half of ``tests/test_gpu_segment_reduce.py``).

For every case the float64 oracle over the stub segment evaluators is the reference; it takes the
generic ``_select`` / ``_regress`` / ``_classify`` path, its scores are fp32 numbers, a plain numpy
restatement of the rules and the torch twin of the kernel (the dry-run ``SegmentedPlan`` fed with
the stand-in segment plans) equal it on every row — validity and fp32 bit patterns — and every
named mutant of the restatement changes at least one row of the case built to catch it."""

import functools

import numpy as np
import pytest
import torch

from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import compile_plan, lowering_dry_run
from tests import _segment_cases as SC

CPU = torch.device("cpu")
NAMES = [c.name for c in SC.all_cases()]


@functools.lru_cache(maxsize=None)
def _restated(name):
    return SC.restate(SC.case(name))


def _twin(case):
    with lowering_dry_run():
        plan = compile_plan(SC.compiled(case.txt), CPU)
    return SC.run_plan(plan, case, CPU, mirrors=True)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_restatement_and_twin_agree(name):
    case = SC.case(name)
    with SC.stubbed(case) as c:  # the generic aggregation path, not the native forest / vote passes
        assert c.evaluator.native_vote() is None and c.evaluator.native_forest() is None
        assert all(isinstance(sub, SC.StubEvaluator) for sub in c.evaluator.sub)
    ref, vref = SC.reference(case)
    fin = vref & np.isfinite(ref)
    if not case.classification and case.method in ("average", "weightedAverage"):
        # one correctly rounded float64 division of two exact sums: not an fp32 number, but the same
        # float64 on both sides (the restatement below equals it in float64), rounded to fp32 once
        assert np.all(np.abs(ref[fin]) <= 64)
    else:
        assert np.array_equal(ref[fin].astype(np.float32).astype(np.float64), ref[fin])
        assert np.all(np.abs(ref[fin]) < 2 ** 23)
    assert np.isinf(ref[vref & ~fin]).all()
    s, v, _ = _restated(name)
    SC.assert_same(s, v, ref, vref, f"{name}: numpy restatement")
    assert np.array_equal(s[vref], ref[vref])  # in float64 too
    s, v, s2, v2 = _twin(case)
    SC.assert_same(s, v, ref, vref, f"{name}: torch twin")
    assert np.array_equal(SC.bits(s2), SC.bits(s)) and np.array_equal(v2, v)


def _stat(names, key):
    return sum(_restated(n)[2][key] for n in names)


def test_every_edge_is_populated():
    by = lambda *parts: [n for n in NAMES if all(p in n.split("-") or p in n for p in parts)]  # noqa: E731
    # an applying segment that returns nothing, under each treatment; validity depends on the treatment
    for m, cls in [(m, False) for m in SC.REG_METHODS] + [(m, True) for m in SC.CLS_METHODS]:
        v = {}
        for t in SC.TREATMENTS:
            case = SC.states_case(m, cls, t)
            assert _restated(case.name)[2]["nothing"] >= 700, case.name
            v[t] = SC.reference(case)[1]
            assert 0 < v[t].mean() < 1
        assert np.array_equal(v[None], v["returnMissing"])
        if m != "selectFirst":  # selectFirst takes the first applying segment under every treatment
            assert (v[None] != v["skipSegment"]).sum() >= 100, m
            assert not (v[None] & ~v["skipSegment"]).any()
    assert _stat(["states-reg-weightedMedian-None", "values-weightedMedian"], "half_wmedian") >= 50
    assert _stat(["states-reg-median-skipSegment", "values-median"], "even_median") >= 50
    for m in SC.VOTE_METHODS + SC.PROB_METHODS:
        for n in (f"classes-{m}", f"classes-{m}-perm", f"states-cls-{m}-skipSegment"):
            assert _restated(n)[2]["top_tie"] >= 10, n
    for n in by("target", "round"):
        assert _restated(n)[2]["half_round"] >= 20, n
    for n in by("target"):  # rows without an applying segment, rows without a prediction
        case = SC.case(n)
        assert ((case.X > 0).sum(axis=1) == 0).sum() >= 4
    # the sizes: each single-bit row kind, all and none, at every K
    for K in SC.SIZES:
        case = SC.size_case(K, "sum", False)
        a = case.X > 0
        one = a.sum(axis=1) == 1
        for seg in {0, K - 1, min(63, K - 1), min(64, K - 1)}:
            assert (one & a[:, seg]).sum() >= 15, (K, seg)
        assert a.all(axis=1).sum() >= 15 and (~a.any(axis=1)).sum() >= 15
    # both non-applying spellings, everywhere
    for n in NAMES:
        X = SC.case(n).X
        assert (X == -1).any() and np.isnan(X).any() and (X == 1).any(), n
    # a prescribed infinity decides rows of every infinite case, and the oracle keeps some of them
    assert np.isinf(SC.reference(SC.case("inf-selectFirst"))[0]).any()


CATCHES = {
    "wmedian-le": ["states-reg-weightedMedian-None", "values-weightedMedian"],
    "median-lower": ["states-reg-median-skipSegment", "values-median", "classes-median"],
    "ties-high": [f"classes-{m}" for m in SC.VOTE_METHODS + SC.PROB_METHODS] + ["size-K65-majorityVote",
                                                                                  "classes-max-perm"],
    "skip-inverted": ["states-reg-sum-None", "states-reg-sum-skipSegment", "states-cls-majorityVote-returnMissing",
                      "states-cls-median-skipSegment", "size-K129-sum"],
    "select-fallthrough": ["states-reg-selectFirst-None", "states-cls-selectFirst-skipSegment",
                           "target-reg-selectFirst-None-clip-default"],
    "round-half-even": ["target-reg-selectFirst-None-round", "target-reg-median-skipSegment-round"],
}


@pytest.mark.parametrize("mutant", list(CATCHES))
def test_named_mutants_change_a_row(mutant):
    """A rule restated wrongly must show on the cases meant to catch it; a mutant no row detects
    means the cases are too weak, not that the kernel is right."""
    for name in CATCHES[mutant]:
        ref, vref = SC.reference(SC.case(name))
        s, v, _ = SC.restate(SC.case(name), mutant)
        changed = (v != vref) | (vref & v & (SC.bits(s) != SC.bits(ref)))
        assert changed.sum() >= 1, (mutant, name)
        print(f"{mutant}: {int(changed.sum())} of {len(v)} rows of {name}")


def test_unstable_sort_cannot_show():
    """The order among EQUAL values cannot change a weighted median (module docstring of
    ``_segment_cases``): reversing it changes no row, although equal values are everywhere."""
    for name in ["states-reg-weightedMedian-None", "values-weightedMedian"]:
        case = SC.case(name)
        use = (case.X > 0).T & case.V.astype(bool) & ~np.isnan(case.S)
        ties = sum(len(set(case.S[use[:, r], r])) < use[:, r].sum() for r in range(case.n))
        assert ties >= 50
        s, v, _ = SC.restate(case, "unstable-sort")
        SC.assert_same(s, v, *SC.reference(case), f"{name}: unstable sort")


# --------------------------------------------------------------------------- real segment trees


class _OracleSegment:
    """Stand-in segment plan over the real segment evaluator (as tests/test_segmented.py)."""

    def __init__(self, compiled, sub):
        self.c, self.sub = compiled, sub

    def launch(self, X, score, valid, stream=None, probs=None, **kw):
        r = self.sub.evaluate(self.c.columns(X.double().numpy()))
        score.copy_(torch.from_numpy(np.where(r.valid, r.value, np.nan)).float())
        valid.copy_(torch.from_numpy(r.valid.astype(np.uint8)))
        if probs is not None:
            probs.copy_(torch.from_numpy(r.probs).float())


@pytest.mark.parametrize("method,classification", SC.REAL)
def test_real_documents_yield_nothing_and_stay_exact(method, classification):
    """The ``nullPrediction`` documents the GPU test scores through the real tree kernels: exact in
    fp32, partly valid, validity depends on the treatment, and the twin equals the oracle."""
    vrefs = {}
    for t in SC.TREATMENTS:
        txt = SC.real_doc(method, classification, t)
        c = CompiledPmml.from_string(txt)
        assert c.evaluator.native_vote() is None and c.evaluator.native_forest() is None
        X = SC.real_inputs(txt)
        ref, vref = c.score_matrix_oracle(X)
        ok = vref & np.isfinite(ref)
        if classification or method not in ("average", "weightedAverage"):  # those: one division of exact sums
            assert np.array_equal(ref[ok].astype(np.float32).astype(np.float64), ref[ok])
        assert 0 < vref.mean() < 1
        vrefs[t] = vref
        with lowering_dry_run():
            plan = compile_plan(c, CPU)
            each = compile_plan(c, CPU, layout="perfect")
        seg = SC.segmented(plan)
        # the two lowerings the GPU test runs: pointer-layout members of one launch, a launch each
        assert all(p.layout == "pointer" for p in seg.subs) and seg.skip == (t == "skipSegment")
        assert all(p.layout == "perfect" for p in SC.segmented(each).subs)
        seg.subs = [_OracleSegment(c, sub) for sub in c.evaluator.sub]
        s, v = torch.empty(len(X)), torch.empty(len(X), dtype=torch.uint8)
        plan.launch(torch.from_numpy(np.array(X)), s, v)
        SC.assert_same(s.numpy(), v.numpy().astype(bool), ref, vref, f"{method} {t}")
    if method != "selectFirst":
        assert (vrefs[None] != vrefs["skipSegment"]).any()
