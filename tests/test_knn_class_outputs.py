"""Class outputs of k-NN classifiers without a GPU: the float64 reference of ``_knn_vote_cases``
against the oracle, the fp32 twin and its mutants, the dry-run ``OutputPlan(knn_classes=True)``
against ``outputs_matrix_oracle``, the switch, the 1-NN tables, the limits, and the share of rows the
GPU comparisons of the inexact documents leave out."""

import os

import numpy as np
import pytest

import _entity_cases as EC
import _knn_vote_cases as VC
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.bench import synth
from flink_jpmml_amd.runtime.outputs import oracle_outputs, oracle_top_k
from flink_jpmml_amd.runtime.plans import NotLowerable, lowering_dry_run

ROWS = 21
TOP = 3


def _same(a, b) -> bool:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def exact():
    """name -> (case, compiled, rows, oracle (s, v, cols, res, ok), reference (label, valid, shares))."""
    out = {}
    for name, c in VC.EXACT.items():
        compiled = PmmlModel.from_string(VC.document(c, VC.class_outputs(c))).compiled
        X = VC.rows(c, ROWS)
        out[name] = (c, compiled, X, oracle_outputs(compiled, X, top_k=TOP), VC.reference(c, X))
    return out


@pytest.mark.parametrize("name", sorted(VC.EXACT))
def test_reference_equals_the_oracle(exact, name):
    c, compiled, X, (s, v, cols, res, ok), (lab, valid, shares) = exact[name]
    assert list(res.categories) == c["categories"]
    assert np.array_equal(valid, np.asarray(res.valid, dtype=bool) & ok)
    assert _same(lab, res.value) and _same(shares, res.probs)
    ti, tp = oracle_top_k(res.probs, valid, TOP)
    wi, wp = VC.top_k(shares, valid, TOP)
    assert np.array_equal(ti, wi) and _same(tp, wp)
    # the probes hold what they promise
    assert np.isnan(X).all(axis=1).any() and not valid[np.isnan(X).all(axis=1)].any()
    assert np.isnan(shares[~valid]).all() and (np.abs(shares[valid].sum(axis=1) - 1.0) < 1e-15).all()
    assert c["weighted"] or (np.isnan(X).any(axis=1) & valid).any()


def test_cases_hold_the_promised_votes():
    c = VC.EXACT["hand5_majority_sq"]
    lab, valid, sh = VC.reference(c, VC.rows(c, 4))
    assert sorted(sh[0][sh[0] > 0]) == [0.2, 0.4, 0.4] and c["categories"][int(lab[0])] == "B"  # 2-2-1, B first
    assert c["categories"] == ["A", "B", "C", "D", "E"] and "D" not in c["targets"] and "E" not in c["declared"]
    w = VC.EXACT["hand5_weighted_sq"]
    lab, _, sh = VC.reference(w, VC.rows(w, 4))
    assert sh[1][0] == sh[1][1] == 1 / 2.25 and w["categories"][int(lab[1])] == "B"  # 1 against 1/2 + 1/2
    d = np.sort(np.abs(c["inst"] - VC.base_point(2)).sum(axis=1))
    assert d[3] == d[4] == d[5] == 3  # the k-th and (k+1)-th distances tie
    t0 = VC.EXACT["hand3_t0_weighted_sq"]
    _, _, sh = VC.reference(t0, VC.rows(t0, 3))
    assert sorted(sh[1]) == [0, 0, 0, 0.5, 0.5] and sorted(sh[2]) == [0, 0, 0, 0, 1]  # two and one exact matches
    big = VC.EXACT["c40k3_majority"]
    assert len(big["categories"]) == 40 > big["k"]


@pytest.mark.parametrize("name", sorted(VC.EXACT))
def test_twin_equals_the_reference_bit_for_bit(exact, name):
    c, _, X, _, (lab, valid, shares) = exact[name]
    tl, tv, ts = VC.twin(c, X)
    assert np.array_equal(tv, valid) and _same(tl, lab)
    assert np.array_equal(VC.bits(ts), VC.bits(shares.astype(np.float32)))


@pytest.mark.parametrize("mutant", VC.MUTANTS)
def test_every_mutant_changes_a_compared_bit(exact, mutant):
    hit = []
    for name, (c, _, X, _, (lab, valid, shares)) in exact.items():
        tl, _, ts = VC.twin(c, X, mutant)
        if not _same(tl, lab) or not np.array_equal(VC.bits(ts), VC.bits(shares.astype(np.float32))):
            hit.append(name)
    assert hit, mutant


def _plan(compiled, **kw):
    with lowering_dry_run():
        return compiled.output_plan("cpu", knn_classes=True, **kw)


def _assert_plan_matches(compiled, X, top=TOP):
    """The dry-run plan's columns, score, validity and top-k against the oracle's, as fp32 bits."""
    s, v, cols, res, ok = oracle_outputs(compiled, X, top_k=top)
    plan = _plan(compiled, top_k=top)
    sc, va, mat = plan.score_outputs(X)
    sc, va, mat = sc.numpy(), va.numpy(), mat.numpy()
    assert np.array_equal(va, v) and np.array_equal(VC.bits(sc), VC.bits(s))
    for i, n in enumerate(plan.names):
        assert np.array_equal(VC.bits(mat[:, i]), VC.bits(cols[n])), n
    ti, tp = oracle_top_k(res.probs, np.asarray(res.valid, dtype=bool) & ok, top)
    w = len(plan.names)
    assert np.array_equal(np.nan_to_num(mat[:, w: w + top], nan=-1).astype(np.int64), ti)
    assert np.array_equal(VC.bits(mat[:, w + top:]), VC.bits(tp))
    return plan


@pytest.mark.parametrize("name", sorted(VC.EXACT))
def test_dry_run_plan_gives_the_oracles_columns(exact, name):
    c, compiled, X, _, _ = exact[name]
    plan = _assert_plan_matches(compiled, X)
    assert plan.labels == c["categories"] and plan.C == len(c["categories"])
    with lowering_dry_run():
        assert plan.inner.class_table is None and compiled.plan("cpu").class_table is not None  # the scoring plan stays


def test_dry_run_plan_numeric_targets_and_entity_fields_together():
    c = VC.EXACT["n33k9_weighted"]
    fields = VC.class_outputs(c, "integer") + [
        '<OutputField name="near" feature="entityId" rank="2" optype="categorical" dataType="string"/>']
    compiled = PmmlModel.from_string(VC.document(c, fields)).compiled
    X = VC.rows(c, ROWS)
    with lowering_dry_run():
        with pytest.raises(NotLowerable, match="'near'"):
            compiled.output_plan("cpu", knn_classes=True)
        plan = compiled.output_plan("cpu", knn_classes=True, entity_ranks=True)
    assert plan.entities is not None
    _, _, cols = compiled.outputs_matrix_oracle(X)
    mat = plan.score_outputs(X)[2].numpy()
    for i, n in enumerate(plan.names):
        assert np.array_equal(VC.bits(mat[:, i]), VC.bits(cols[n])), n


@pytest.mark.parametrize("name", sorted(VC.inexact()))
def test_dry_run_plan_on_the_inexact_documents(name):
    spec = VC.inexact()[name]
    cats = [str(x) for x in range(spec["classes"])]
    c = dict(categories=cats)
    compiled = PmmlModel.from_string(VC.with_outputs(spec["text"], VC.class_outputs(c))).compiled
    _assert_plan_matches(compiled, VC.inexact_rows(200))


# --------------------------------------------------------------------------- the switch


def _refused(text: str, **kw) -> str:
    compiled = PmmlModel.from_string(text).compiled
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        compiled.output_plan("cpu", **kw)
    return str(e.value)


def _lab(kind: str = "predictedValue", extra: str = "") -> str:
    return f'<OutputField name="lab" feature="{kind}"{extra} dataType="string" optype="categorical"/>'


def test_switch_off_refuses_as_before():
    knn = synth.knn_pmml(n_instances=40, k=3)
    no_index = "KnnPlan has no index mode (class / entity outputs are host-only)"
    assert _refused(VC.with_outputs(knn, [_lab()])) == f"output 'lab': {no_index}"
    assert _refused(VC.with_outputs(knn, [_lab("probability")])) == f"output 'lab': {no_index}"
    assert _refused(VC.with_outputs(knn, [_lab("probability", ' value="1"')])) == f"output 'lab': {no_index}"
    assert _refused(knn, top_k=2) == "top_k: KnnPlan does not expose class probabilities"
    near = '<OutputField name="near" feature="entityId" dataType="string" optype="categorical"/>'
    assert _refused(VC.with_outputs(knn, [near, _lab()]), entity_ranks=True) == f"output 'lab': {no_index}"
    one = synth.knn_pmml(n_instances=40, k=1)
    assert _refused(VC.with_outputs(one, [_lab("probability")])) == \
        "output 'lab': ClusterPlan does not expose probabilities"
    assert _refused(one, top_k=2) == "top_k: ClusterPlan does not expose class probabilities"


def test_switch_is_part_of_the_cache_key_and_the_config():
    from flink_jpmml_amd.config import ScoringConfig

    compiled = PmmlModel.from_string(VC.with_outputs(synth.knn_pmml(n_instances=40, k=3), [_lab()])).compiled
    with lowering_dry_run():
        with pytest.raises(NotLowerable):
            compiled.output_plan("cpu")
        b = compiled.output_plan("cpu", knn_classes=True)
        assert compiled.output_plan("cpu", knn_classes=True) is b
        assert compiled.output_plan("cpu", knn_classes=True, entity_ranks=True) is not b
        with pytest.raises(NotLowerable):
            compiled.output_plan("cpu")
    assert ScoringConfig().knn_classes is False and ScoringConfig(knn_classes=True).knn_classes is True
    old = os.environ.get("FJA_KNN_CLASSES")
    try:
        os.environ["FJA_KNN_CLASSES"] = "1"
        assert ScoringConfig.from_env().knn_classes is True
        os.environ["FJA_KNN_CLASSES"] = "0"
        assert ScoringConfig.from_env().knn_classes is False
    finally:
        if old is None:
            os.environ.pop("FJA_KNN_CLASSES", None)
        else:
            os.environ["FJA_KNN_CLASSES"] = old


def test_other_models_ignore_the_switch():
    X = np.random.default_rng(0).standard_normal((9, 4)).astype(np.float32)
    for text in (synth.iris_logistic_pmml(), synth.knn_pmml(40, 4, k=3, classification=False)):
        compiled = PmmlModel.from_string(text).compiled
        with lowering_dry_run():
            a, b = compiled.output_plan("cpu"), compiled.output_plan("cpu", knn_classes=True)
        assert np.array_equal(a.prog_np, b.prog_np) and a.C == b.C and not b._knn_index and not b._knn_one
        assert np.array_equal(VC.bits(a.score_outputs(X)[0].numpy()), VC.bits(b.score_outputs(X)[0].numpy()))


def test_regression_plan_refuses_probs():
    import torch

    compiled = PmmlModel.from_string(synth.knn_pmml(40, 4, k=3, classification=False)).compiled
    with lowering_dry_run():
        plan = compiled.plan("cpu")
    X = torch.zeros((2, 4))
    with pytest.raises(ValueError, match="no class vote shares"):
        plan.launch(X, torch.zeros(2), torch.zeros(2, dtype=torch.uint8), probs=torch.zeros((2, 3)))


# --------------------------------------------------------------------------- 1-NN, limits


def test_one_nn_probabilities_are_tables_over_the_instances():
    text = VC.with_outputs(synth.knn_pmml(n_instances=40, k=1, classes=3),
                           VC.class_outputs(dict(categories=["0", "1", "2"])))
    compiled = PmmlModel.from_string(text).compiled
    X = VC.inexact_rows(64)
    X[5] = np.nan
    plan = _plan(compiled)
    assert type(plan.inner).__name__ == "ClusterPlan" and plan.C is None
    ops = {n: tuple(plan.prog_np[i][:2]) for i, n in enumerate(plan.kernel_names)}
    from flink_jpmml_amd.ops import outputs as K

    assert all(ops[n] == (K.OP_TABLE, 40) for n in ("lab", "pwin", "p_0", "p_2")) and ops["p_nobody"][0] == K.OP_CONST
    _, _, cols = compiled.outputs_matrix_oracle(X)
    mat = plan.score_outputs(X)[2].numpy()
    for i, n in enumerate(plan.names):
        assert np.array_equal(VC.bits(mat[:, i]), VC.bits(cols[n])), n
    assert set(np.unique(cols["p_1"][~np.isnan(cols["p_1"])])) == {0.0, 1.0}
    msg = _refused(text, knn_classes=True, top_k=2)
    assert msg.startswith("top_k: a 1-NN classifier runs on ClusterPlan") and "host-only" in msg


def test_more_than_256_classes_names_the_first_class_field():
    c = VC.generated(65, 3, 257)
    near = '<OutputField name="near" feature="entityId" optype="categorical" dataType="string"/>'
    text = VC.document(c, [near] + VC.class_outputs(c)[:3])
    assert _refused(text, knn_classes=True, entity_ranks=True) == "output 'lab': 257 classes > 256"
    assert _refused(VC.document(c), knn_classes=True, top_k=2) == "top_k: 257 classes > 256"
    ok = VC.generated(65, 3, 256)
    assert _plan(PmmlModel.from_string(VC.document(ok, VC.class_outputs(ok))).compiled, top_k=2).C == 256


# --------------------------------------------------------------------------- what the GPU comparisons leave out


@pytest.mark.parametrize("name", ["knn64k5", "knn200k9"])
def test_inexact_comparisons_leave_out_few_rows(name):
    """From the oracle alone: the share comparison of the unweighted documents leaves out at most
    0.5 % of the rows (an undecided k-th / (k+1)-th neighbour), the label comparison at most 5 %
    (any rank <= k undecided), and fewer than 0.5 % of the weighted rows have their two largest vote
    totals closer than 1e-4. Measured on these documents (the generator's default seed): 0.1 % / 0.3 %
    at k = 5 and 0.4 % / 0.7 % at k = 9; other seeds of the 200 x 4 document range from 0.2 % to 0.8 %
    for the shares, so that bound is a property of this document, not of every one."""
    X = VC.inexact_rows(1000)
    spec = VC.inexact()[name + "_majority"]
    k = spec["k"]
    und = EC.undecided(PmmlModel.from_string(spec["text"]).compiled, X, list(range(1, k + 1)))
    print(name, "shares left out", und[k - 1].mean(), "labels left out", und.any(axis=0).mean())
    assert und[k - 1].mean() <= 0.005
    assert und.any(axis=0).mean() <= 0.05
    res = oracle_outputs(PmmlModel.from_string(VC.inexact()[name + "_weighted"]["text"]).compiled, X, top_k=2)[3]
    top = np.sort(np.asarray(res.probs), axis=1)
    close = ((top[:, -1] - top[:, -2]) < 1e-4).mean()
    print(name, "weighted totals closer than 1e-4", close)
    assert close < 0.005
