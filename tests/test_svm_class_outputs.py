"""Class outputs of SVM classifiers without a GPU: the host oracle against the independent float64
reference of ``_svm_vote_cases`` (label, validity, every vote share, the NaN rows and the rows on which
no machine votes), the dry-run ``OutputPlan(svm_classes=True)`` on each of the three SVM plans, the
tensor program of ``SvmGemmPlan`` on CPU tensors, the refusals, and what must not change:
``ModelResult.probs`` of an SVM and a segmentation over SVM segments."""

import os

import numpy as np
import pytest

import _exact as E
import _svm_vote_cases as SC
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.models.base import class_probabilities
from flink_jpmml_amd.runtime.outputs import oracle_outputs, oracle_top_k
from flink_jpmml_amd.runtime.plans import NotLowerable, lowering_dry_run

ROWS = E.SVM_ROWS
TOP = 3
GUARD = 7.0
NO_INDEX = "has no index mode (class / entity outputs are host-only)"


def _same(a, b) -> bool:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _base(plan):
    while getattr(plan, "inner", None) is not None:
        plan = plan.inner
    return plan


@pytest.fixture(scope="module")
def cases():
    """name -> (case, model, rows, oracle (s, v, cols, res, ok), reference (label, valid, shares, total))."""
    out = {}
    for name in SC.ALL_NAMES:
        c = SC.case(name)
        model = PmmlModel.from_string(c.pmml(SC.class_outputs(c)))
        X = SC.rows(c, ROWS)
        out[name] = (c, model, X, oracle_outputs(model.compiled, X, top_k=TOP), SC.reference(c, X))
    return out


@pytest.mark.parametrize("name", SC.ALL_NAMES)
def test_oracle_equals_the_reference(cases, name):
    c, model, X, (s, v, cols, res, ok), (lab, valid, shares, total) = cases[name]
    compiled = model.compiled
    assert list(res.categories) == c.categories
    assert res.probs is None  # an SVM result keeps no probabilities: segment aggregation sees none
    assert np.array_equal(valid, np.asarray(res.valid, dtype=bool) & ok)
    P = class_probabilities(res)
    assert _same(lab, res.value) and _same(shares, P)
    assert np.isnan(shares[~valid]).all() and not valid.all() and valid.mean() > 0.95
    voted = valid & (total > 0)
    assert (np.abs(shares[voted].sum(axis=1) - 1.0) < 1e-12).all()
    assert np.isnan(shares[valid & (total == 0)]).all()
    # every Output column, through oracle_outputs and outputs_matrix_oracle
    want = SC.expected_columns(c, compiled.schema, X)
    _, _, cols2 = compiled.outputs_matrix_oracle(X)
    for n in cols:
        assert _same(cols[n], want[n]) and _same(cols2[n], want[n]), n
    # host predict_batch_outputs: the matrix, the label strings, top-k
    hs, hv, host = model.predict_batch_outputs(X, top_k=TOP)
    for n in host.names:
        assert _same(host[n], want[n]), n
    labels = [c.categories[int(x)] if o else None for x, o in zip(np.nan_to_num(lab), valid)]
    assert [None if x is None else str(x) for x in host.decode("lab")] == labels
    wi, wp = SC.top_k(shares, valid, TOP)
    wi = np.where(np.isnan(wp), -1, wi)  # NaN shares (no machine voted) are never selected
    assert np.array_equal(host.top_index, wi) and _same(host.top_probability, wp)
    ti, tp = oracle_top_k(P, valid, TOP)
    assert np.array_equal(ti, wi) and _same(tp, wp)


@pytest.mark.parametrize("name", ["str-ovo3", "oaa-noalt", "maxwins"])
def test_single_records_report_the_shares(cases, name):
    c, model, X, _, (lab, valid, shares, total) = cases[name]
    picks = list(np.nonzero(valid & (total > 0))[0][:3]) + list(np.nonzero(valid & (total == 0))[0][:2]) + \
        list(np.nonzero(~valid)[0][:1])
    for r in picks:
        outs = model.predict_with_outputs(X[r].astype(np.float64)).outputs
        if not valid[r]:
            assert not outs or outs.get("pwin") is None or np.isnan(outs["pwin"])
            continue
        j = int(lab[r])
        assert str(outs["lab"]) == c.categories[j]
        assert _same(outs["pwin"], shares[r, j]) and _same(outs[f"p_{c.categories[0]}"], shares[r, 0])


def test_cases_hold_what_they_promise(cases):
    for name in SC.NO_VOTE_CASES:
        _, _, _, _, (lab, valid, shares, total) = cases[name]
        none = valid & (total == 0)
        assert none.sum() >= 5 and (lab[none] == 0).all(), name  # valid, class 0, no shares
    ties = {}
    for name in SC.PROBE_NAMES:
        c, _, X, _, (_, valid, _, _) = cases[name]
        v = c.votes(X)[0]
        ties[name] = ((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1)[valid].mean()
        if c.n_classes > 2:
            assert 0.10 < ties[name] < 0.50, (name, ties[name])  # the tie rule is exercised
    print({k: round(float(t), 3) for k, t in ties.items()})
    assert cases["str-ovo3"][0].categories == ["ant", "bee", "cat", "late"]
    big = cases["m128c256"][0]
    assert big.n_classes == 256 and len(big.machines) == 128
    lim = cases["m8c16"][0]
    assert lim.n_classes == 16 and len(lim.machines) == 8 and lim.n_sv >= 32 > cases["m8c16-valu"][0].n_sv
    g = cases["gemm-m9c18"][0]
    assert g.n_classes > 16 and len(g.machines) > 8


# --------------------------------------------------------------------------- lowering dry run


@pytest.mark.parametrize("name", SC.ALL_NAMES)
def test_dry_run_plan_gives_the_oracles_columns(cases, name):
    c, model, X, (s, v, cols, res, ok), (lab, valid, shares, total) = cases[name]
    compiled = model.compiled
    with lowering_dry_run():
        plan = compiled.output_plan("cpu", svm_classes=True, top_k=TOP, svm_impl=c.impl)
        scoring = compiled.plan("cpu", svm_impl=c.impl)
    base = _base(plan.inner)
    assert type(base).__name__ == c.plan and base.table is None  # index mode
    assert _base(scoring).table is not None  # the cached scoring plan stays as it is
    assert plan.labels == c.categories and plan.C == c.n_classes and plan._svm_index
    sc, va, mat = plan.score_outputs(X)
    sc, va, mat = sc.numpy(), va.numpy(), mat.numpy()
    assert np.array_equal(va, v) and np.array_equal(SC.bits(sc), SC.bits(s))
    if c.target_type == "string":
        assert not v.any()  # the labels are no numbers: EmptyScore on the scoring side
    for i, n in enumerate(plan.names):
        assert np.array_equal(SC.bits(mat[:, i]), SC.bits(cols[n])), n
    ti, tp = oracle_top_k(class_probabilities(res), valid, TOP)
    w = len(plan.names)
    assert np.array_equal(np.nan_to_num(mat[:, w: w + TOP], nan=-1).astype(np.int64), ti)
    assert np.array_equal(SC.bits(mat[:, w + TOP:]), SC.bits(tp))
    # the raw results the kernels must leave: index, validity, fp32 shares
    raw_s, raw_v, probs, _ = plan.raw_from_oracle(X.astype(np.float32))
    assert np.array_equal(SC.bits(probs), SC.bits(shares.astype(np.float32)))
    assert np.array_equal(raw_v != 0, valid) and np.array_equal(SC.bits(raw_s), SC.bits(lab))


# --------------------------------------------------------------------------- SvmGemmPlan on CPU tensors


@pytest.mark.parametrize("name", ["gemm-m9c18", "oaa-noalt", "maxwins", "wide-17cls", "mfma-33sv"])
def test_gemm_plan_shares_and_index_on_cpu_tensors(cases, name):
    import torch

    c, model, X, _, (lab, valid, shares, total) = cases[name]
    compiled = model.compiled
    with lowering_dry_run():
        plan = compiled.output_plan("cpu", svm_classes=True, svm_impl="gemm")
        scoring = compiled.plan("cpu", svm_impl="gemm")
    gemm = _base(plan.inner)
    assert type(gemm).__name__ == "SvmGemmPlan" and gemm.table is None
    n, C = len(X), c.n_classes
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    buf = torch.full((n + 2, C), GUARD, dtype=torch.float32)
    score, ok = torch.empty(n), torch.empty(n, dtype=torch.uint8)
    gemm.launch(Xt, score, ok, probs=buf[1: n + 1])
    assert (buf[0] == GUARD).all() and (buf[-1] == GUARD).all()
    assert np.array_equal(SC.bits(buf[1:-1].numpy()), SC.bits(shares.astype(np.float32)))
    assert np.array_equal(ok.numpy() != 0, valid) and np.array_equal(SC.bits(score.numpy()), SC.bits(lab))
    # with its table the same program still scores as before, and writes the same shares
    gs = _base(scoring)
    buf2 = torch.full((n, C), GUARD, dtype=torch.float32)
    s2, v2 = torch.empty(n), torch.empty(n, dtype=torch.uint8)
    gs.launch(Xt, s2, v2, probs=buf2)
    s0, v0 = torch.empty(n), torch.empty(n, dtype=torch.uint8)
    gs.launch(Xt, s0, v0)
    assert np.array_equal(SC.bits(s2.numpy()), SC.bits(s0.numpy())) and np.array_equal(v2.numpy(), v0.numpy())
    if c.target_type != "string":
        assert np.array_equal(SC.bits(buf2.numpy()), SC.bits(shares.astype(np.float32)))
    with pytest.raises(ValueError, match="needs probs"):
        gemm.launch(Xt, score, ok)


# --------------------------------------------------------------------------- refusals, the switch


def _refused(text: str, **kw) -> str:
    compiled = PmmlModel.from_string(text).compiled
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        compiled.output_plan("cpu", **kw)
    return str(e.value)


@pytest.mark.parametrize("name,plan", [("str-ovo3", "SvmPlan"), ("m128c256", "SvmWidePlan"),
                                       ("gemm-m9c18", "SvmGemmPlan")])
def test_switch_off_names_the_field(name, plan):
    c = SC.case(name)
    fields = SC.class_outputs(c)
    for f, fname in ((fields[0], "lab"), (fields[2], "pwin"), (fields[3], f"p_{c.categories[0]}")):
        assert _refused(c.pmml([f]), svm_impl=c.impl) == f"output {fname!r}: {plan} {NO_INDEX}"
    assert _refused(c.pmml(), top_k=2, svm_impl=c.impl) == f"top_k: {plan} does not expose class probabilities"
    # the k-NN switch is not the SVM switch
    assert _refused(c.pmml(fields[:1]), knn_classes=True, svm_impl=c.impl) == f"output 'lab': {plan} {NO_INDEX}"


def test_rank_above_one_stays_refused():
    c = SC.case("str-ovo3")
    f = '<OutputField name="second" feature="predictedValue" rank="2" optype="categorical" dataType="string"/>'
    assert "rank 2 > 1" in _refused(c.pmml([f]), svm_classes=True)


def test_more_than_256_classes_names_the_field():
    L = [f"k{i}" for i in range(258)]
    c = SC.VoteCase("c258", 8, 12, [(L[2 * m], L[2 * m + 1]) for m in range(129)], L, seed=9, impl="gemm",
                    plan="SvmGemmPlan")
    fields = SC.class_outputs(c)
    assert _refused(c.pmml(fields[:3]), svm_classes=True) == "output 'lab': 258 classes > 256"
    assert _refused(c.pmml(fields[2:3]), svm_classes=True) == "output 'pwin': 258 classes > 256"
    assert _refused(c.pmml(), svm_classes=True, top_k=2) == "top_k: 258 classes > 256"
    # the host answers all the same
    X = SC.rows(c, 40)
    _, _, host = PmmlModel.from_string(c.pmml(fields[:3])).predict_batch_outputs(X, top_k=2)
    lab, valid, shares, _ = SC.reference(c, X)
    assert _same(host["pwin"], np.where(valid, shares[np.arange(40), np.nan_to_num(lab).astype(int)], np.nan))


def test_plans_refuse_probs_they_cannot_fill():
    import torch

    from flink_jpmml_amd.bench import synth

    reg = PmmlModel.from_string(synth.svm_pmml(8, 40, classification=False)).compiled
    cls = PmmlModel.from_string(SC.case("m8c16").pmml()).compiled
    X = torch.zeros((5, 8))
    s, v = torch.zeros(5), torch.zeros(5, dtype=torch.uint8)
    for impl in ("fused", "wide", "gemm"):
        with lowering_dry_run():
            rp, cp = _base(reg.plan("cpu", svm_impl=impl)), _base(cls.plan("cpu", svm_impl=impl))
        with pytest.raises(ValueError, match="no class vote shares"):
            rp.launch(X, s, v, probs=torch.zeros((5, 2)))
        with pytest.raises(ValueError, match="contiguous"):
            cp.launch(X, s, v, probs=torch.zeros((5, 32))[:, ::2])
        with pytest.raises(ValueError, match="contiguous"):
            cp.launch(X, s, v, probs=torch.zeros((5, 15)))


def test_regression_svm_and_other_models_ignore_the_switch():
    from flink_jpmml_amd.bench import synth

    X = np.random.default_rng(0).standard_normal((9, 8)).astype(np.float32)
    for text in (synth.svm_pmml(8, 40, classification=False), synth.iris_logistic_pmml()):
        compiled = PmmlModel.from_string(text).compiled
        Xc = X[:, : len(compiled.active_fields)]
        with lowering_dry_run():
            a, b = compiled.output_plan("cpu"), compiled.output_plan("cpu", svm_classes=True)
        assert a is not b and np.array_equal(a.prog_np, b.prog_np) and a.C == b.C and not b._svm_index
        assert np.array_equal(SC.bits(a.score_outputs(Xc)[0].numpy()), SC.bits(b.score_outputs(Xc)[0].numpy()))


def test_switch_is_part_of_the_cache_key_and_the_config():
    from flink_jpmml_amd.config import ScoringConfig

    c = SC.case("str-ovo3")
    compiled = PmmlModel.from_string(c.pmml(SC.class_outputs(c))).compiled
    with lowering_dry_run():
        with pytest.raises(NotLowerable):
            compiled.output_plan("cpu")
        b = compiled.output_plan("cpu", svm_classes=True)
        assert compiled.output_plan("cpu", svm_classes=True) is b
        assert compiled.output_plan("cpu", svm_classes=True, knn_classes=True) is not b
        with pytest.raises(NotLowerable):
            compiled.output_plan("cpu")
    assert ScoringConfig().svm_classes is False and ScoringConfig(svm_classes=True).svm_classes is True
    old = os.environ.get("FJA_SVM_CLASSES")
    try:
        os.environ["FJA_SVM_CLASSES"] = "1"
        assert ScoringConfig.from_env().svm_classes is True
        os.environ["FJA_SVM_CLASSES"] = "0"
        assert ScoringConfig.from_env().svm_classes is False
    finally:
        if old is None:
            os.environ.pop("FJA_SVM_CLASSES", None)
        else:
            os.environ["FJA_SVM_CLASSES"] = old


# --------------------------------------------------------------------------- what must not change


@pytest.mark.parametrize("method", SC.SEGMENT_METHODS)
def test_segmentation_over_svm_segments_is_unchanged(method):
    """``tests/golden/svm_segment_parent.npz`` holds what the host oracle answered for these documents
    before SVM results carried vote shares."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "svm_segment_parent.npz"))
    X = E.svm_matrix(SC.SEGMENT_ROWS, 9, seed=5)
    s, v = PmmlModel.from_string(SC.segmented_document(method)).predict_batch(X)
    assert np.array_equal(np.asarray(v, dtype=bool), gold[method + "_valid"])
    assert _same(s, gold[method + "_score"])


# --------------------------------------------------------------------------- what the GPU comparison leaves out


@pytest.mark.parametrize("kernel", ["polynomial", "radialBasis", "sigmoid"])
def test_inexact_comparison_leaves_out_few_rows(kernel):
    """From the oracle alone: the rows of the polynomial / RBF / sigmoid documents on which some
    machine's decision value is within ``2 * SVM_ULP_CONSTANT * 2^-24 * T`` of its threshold are at most
    10 % of the valid rows (largest: 33 of 499, wide-9cls polynomial; none for any RBF case)."""
    left = {}
    for name in E.NONLINEAR_SVM_CASES:
        if E.SVM_CASES[name][2] < 2:
            continue
        probe, _ = E.svm_probe(name, kernel=kernel)
        X = E.svm_matrix(ROWS, probe.F, seed=6)
        valid = ~np.isnan(X).any(axis=1)
        decided = SC.decided_rows(probe, X)
        left[name] = int((valid & ~decided).sum())
        assert (valid & decided).sum() >= 0.9 * valid.sum(), (name, kernel, left[name], int(valid.sum()))
    print(kernel, left)
    if kernel == "radialBasis":
        assert not any(left.values())
