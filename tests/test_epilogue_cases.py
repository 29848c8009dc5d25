"""CPU side of the exact-eta epilogue probes (tests/_epilogue_cases.py).

The float64 reference equals the oracle on every grid (labels, validity, cast Target values equal,
probabilities to 1e-12); the rows the fp32 model-value rule touches are an exact, constructed set;
the fp32 twin of csrc/epilogue.h equals the reference under that rule; every named mutant of the
twin changes a compared label, validity bit or cast value; the torch twins of the epilogue agree;
and ``LinearPlan`` refuses what linear.hip's launcher refuses."""

import functools

import numpy as np
import pytest
import torch

from tests import _epilogue_cases as E

from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import lowering_dry_run

F32 = np.float32
CASES = {c.name: c for c in E.all_cases()}
GLM = {c.name: c for c in E.glm_cases()}
# numpy's fp32 library functions against the float64 reference: the bound the GPU file may not exceed
C_MAX = 16.0


@functools.lru_cache(maxsize=None)
def compiled(name: str):
    return CompiledPmml.from_string(CASES[name].probe.pmml() if name in CASES else GLM[name].doc)


oracle = E.oracle


def assert_same_decisions(got, ref, what, exact=True):
    """Validity on every row; scores (numeric class labels, ``none`` link values, cast Target
    values: all exact) bit for bit. ``exact=False``: a regression link value, within 1e-12."""
    assert np.array_equal(got["valid"], ref["valid"]), \
        f"{what}: validity differs on rows {np.flatnonzero(got['valid'] != ref['valid'])[:8]}"
    v = ref["valid"]
    if not exact:
        err = np.abs(np.asarray(got["score"], np.float64)[v] - ref["score"][v])
        assert (err <= 1e-12 * np.maximum(1.0, np.abs(ref["score"][v]))).all(), what
        return
    assert np.array_equal(np.asarray(got["score"], F32)[v], np.asarray(ref["score"], F32)[v]), \
        f"{what}: scores differ on rows {np.flatnonzero(v)[np.asarray(got['score'], F32)[v] != np.asarray(ref['score'], F32)[v]][:8]}"


def link_bound(norm: str, ref: np.ndarray, C: float = C_MAX) -> np.ndarray:
    return E.value_bound(norm, ref, C)


def exact_scores(case) -> bool:
    p = case.probe
    return bool(p.K) or p.norm == "none" or bool((p.target or {}).get("cast"))


def expected_flagged(case) -> np.ndarray:
    """The rows of the fp32 model-value rule, from the way the grids were built: the FLT_MAX +
    FLT_MAX rows, and ``exp`` of 89, 100, 104, 120 or of the largest fp32 number near ln(FLT_MAX)."""
    p = case.probe
    eta = case.eta if p.K != 2 else case.eta[:, :1]
    over = np.zeros(eta.shape, bool)
    if p.norm == "none":
        over = np.isfinite(eta) & (np.abs(eta) > E.FLT_MAX)
    if p.norm == "exp":
        over = np.isin(eta, (89.0, 100.0, 104.0, 120.0, E.EXP_EDGE[0]))
    if p.norm in ("softmax", "simplemax"):
        assert not over.any()
    return over.any(axis=1) & ~case.miss


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_oracle(name):
    case = CASES[name]
    c = compiled(name)
    s, v, probs = oracle(c, case.X)
    ref = case.reference(fp32_rule=False)
    assert_same_decisions(dict(score=s, valid=v), ref, name, exact=exact_scores(case))
    assert ref["valid"].any() and (case.probe.target or {}).get("default") is not None or not ref["valid"].all()
    if probs is not None:
        ok = ref["valid"]
        assert np.abs(probs[ok] - ref["probs"][ok]).max() <= 1e-12
    # the fp32 model-value rule touches exactly the constructed rows, and nothing else changes
    ruled = case.reference(fp32_rule=True)
    assert np.array_equal(ref["flagged"], expected_flagged(case))
    fl = ref["flagged"]
    assert np.array_equal(ruled["valid"][~fl], ref["valid"][~fl])
    assert np.array_equal(ruled["score"][~fl], ref["score"][~fl], equal_nan=True)
    default = (case.probe.target or {}).get("default")
    if default is None:
        assert not ruled["valid"][fl].any() and ref["valid"][fl].all()
    else:
        assert ruled["valid"][fl].all() and (ruled["score"][fl] == default).all()


def test_cloglog_low_side_follows_the_oracle_form():
    """cloglog of -100 and of -120: the oracle's ``1 - exp(-e^eta)`` is 0 for both (a tie, first
    class), the cancellation-free form orders them. The twin breaks fp32 ties with the oracle's
    form, so it answers as the oracle does."""
    case = E.low_side_case()
    s, v, _ = oracle(CompiledPmml.from_string(case.probe.pmml()), case.X)
    assert v.all() and len(s) == 4
    tw = case.twin()
    assert np.array_equal(tw["valid"], v) and np.array_equal(tw["score"], s.astype(F32))
    assert not np.array_equal(case.reference(False)["score"], s)


@pytest.mark.parametrize("name", list(GLM))
def test_glm_reference_equals_oracle_and_lowers_dense(name):
    """Ordinal and binomial GLMs over numeric covariates: the reference over the tables the design
    lowering builds equals the GLM oracle, and the plan is a plain ``LinearPlan`` in the expected
    mode (no derive pass in front: every design column is an input field)."""
    case = GLM[name]
    c = compiled(name)
    s, v, probs = oracle(c, case.X)
    ref = case.reference(fp32_rule=False)
    assert_same_decisions(dict(score=s, valid=v), ref, name)
    assert np.abs(probs[v] - ref["probs"][v]).max() <= 1e-12
    assert not ref["flagged"].any()
    with lowering_dry_run():
        plan = PL.compile_plan(c, torch.device("cpu"))
    # the design lowering always wraps a GeneralRegressionModel: a derive pass that copies the
    # covariates, then the dense tables on linear.hip
    assert type(plan).__name__ == "DerivedPlan" and type(plan.inner).__name__ == "LinearPlan"
    plan = plan.inner
    assert plan.epi_args["mode"] == E.epilogue_mode(case.K, case.norm)
    assert plan.epi_args["link"] == E.LINK_ID[case.norm.split(":")[-1]]


@pytest.mark.parametrize("name", list(CASES) + list(GLM))
def test_twin_equals_reference_under_the_fp32_rule(name):
    case = CASES.get(name) or GLM[name]
    ref, tw = case.reference(fp32_rule=True), case.twin()
    norm = case.probe.norm if name in CASES else case.norm
    norm = norm.split(":")[-1]
    if name in GLM or exact_scores(case):
        assert_same_decisions(tw, ref, name)
    else:  # a regression link value: validity here, the value under the bound below
        assert np.array_equal(tw["valid"], ref["valid"])
    v = ref["valid"] & ~ref["flagged"] & np.isfinite(ref["probs"]).all(axis=1)
    err = np.abs(tw["probs"].astype(np.float64)[v] - ref["probs"][v])
    K = case.probe.K if name in CASES else case.K
    mag = E.magnitudes(K, norm, ref["probs"][v])
    assert (err <= link_bound(norm, mag)).all(), float((err / link_bound(norm, mag, 1.0)).max())


def _differs(a, b) -> bool:
    both = a["valid"] & b["valid"]
    return (not np.array_equal(a["valid"], b["valid"])) or not np.array_equal(a["score"][both], b["score"][both])


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_every_mutant_of_the_twin_shows(mutant):
    """Each named mutant changes at least one compared label, validity bit or cast value."""
    hit = [name for name, case in {**CASES, **GLM}.items() if _differs(case.twin(mutant), case.twin())]
    print(mutant, "shows on", len(hit), "grids:", hit[:6])
    assert hit


def test_double_tie_break_is_needed_and_sufficient():
    """EPI_LINKMAX on the saturation pairs: (20, 30) -> the second class, (30, 20) -> the first,
    (40, 50) -> the first (the oracle itself ties), (-120, -100) -> the second. Plain fp32 argmax
    (the twin without its float64 tie-break) gets the first and the last wrong."""
    case = CASES["K3-F63-logit"]
    ref = case.reference(fp32_rule=True)
    eta = case.eta
    want = {(20.0, 30.0): 1, (30.0, 20.0): 0, (40.0, 50.0): 0, (-120.0, -100.0): 1, (-100.0, -120.0): 0}
    for (a, b), lab in want.items():
        for i in (0, 1):
            rows = np.flatnonzero((eta[:, i] == a) & (eta[:, i + 1] == b) & ~case.miss)
            assert len(rows) and (ref["label"][rows] == i + lab).all(), (a, b, i)
    p32 = E.twin_link("logit", eta.astype(F32))
    plain = np.argmax(p32, axis=1)
    rows = np.flatnonzero((eta[:, 0] == 20.0) & (eta[:, 1] == 30.0) & ~case.miss)
    assert len(rows) and (plain[rows] == 0).all() and (case.twin()["label"][rows] == 1).all()


# --------------------------------------------------------------------------- torch twins


@pytest.mark.parametrize("link", E.LINKS)
def test_torch_apply_link_twin(link):
    from flink_jpmml_amd.parallel.tree_shard import apply_link

    y = E.SWEEP[np.abs(E.SWEEP) <= 88]
    got = apply_link(E.LINK_ID[link], torch.from_numpy(y.astype(F32))).numpy().astype(np.float64)
    ref = E.ref_link(link, y)
    assert (np.abs(got - ref) <= link_bound(link, ref)).all()
    if link in E.BOUNDED and link != "cloglog" and link != "loglog":
        assert got[y == 0][0] == 0.5


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.probe.K in (0, 2) and c.probe.norm in E.LINKS])
def test_torch_finish_epilogue_twin(name):
    """``tree_shard.finish_epilogue`` / ``plans.apply_target_torch`` (single-accumulator epilogues:
    regression and the two-table rule) on the plan's own epilogue arguments. Validity on every row;
    scores bit for bit where the arithmetic is exact (class labels, link ``none``, every cast Target
    value, also after a link), else a link value within the bound."""
    from flink_jpmml_amd.parallel.tree_shard import finish_epilogue

    case = CASES[name]
    with lowering_dry_run():
        plan = PL.LinearPlan(compiled(name), torch.device("cpu"))
    with np.errstate(over="ignore"):
        raw = torch.from_numpy(case.eta[:, 0].astype(F32))
    s, ok = finish_epilogue(raw, torch.from_numpy(~case.miss), plan.epi_args,
                            labels=E.class_labels(2) if case.probe.K else None)
    ref = case.reference(fp32_rule=True)
    got, v = s.numpy(), ref["valid"]
    assert np.array_equal(ok.numpy(), v)
    assert np.isnan(got[~v]).all()
    if exact_scores(case):
        assert np.array_equal(got[v], ref["score"][v].astype(F32))
    else:
        assert not case.probe.target  # a link value, un-cast: no Target shape of the grids leaves one
        err = np.abs(got[v].astype(np.float64) - ref["score"][v])
        assert (err <= link_bound(case.probe.norm, ref["score"][v])).all()


# --------------------------------------------------------------------------- lowering limits


@pytest.mark.parametrize("K,F,lowers", [(17, 34, False), (2, 129, False), (16, 128, True)])
def test_linear_plan_refuses_what_the_launcher_refuses(K, F, lowers):
    """linear.hip holds 16 tables and 128 fields; beyond, the plan must say so at bind time
    (``NotLowerable``, which the fallback policy sees), not fail at the first batch."""
    c = CompiledPmml.from_string(E.Probe(F, K, "softmax").pmml())
    with lowering_dry_run():
        if lowers:
            plan = PL.LinearPlan(c, torch.device("cpu"))
            assert plan.K == K and plan.W.shape == (F, K) and plan.listed is None
        else:
            with pytest.raises(PL.NotLowerable):
                PL.LinearPlan(c, torch.device("cpu"))


def test_listed_mask_marks_the_predictors_a_table_names():
    """A sparse document lowers with a ``listed`` mask (bit k of word f: table k names field f); an
    explicit coefficient of 0 is listed."""
    p = E.Probe(3, 3, "logit", sparse=True, zero_coef=(1, 0))
    with lowering_dry_run():
        plan = PL.LinearPlan(CompiledPmml.from_string(p.pmml()), torch.device("cpu"))
    assert plan.listed.tolist() == [1, 2 | 1, 4]
