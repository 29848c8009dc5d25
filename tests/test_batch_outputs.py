"""PMML Output fields and top-k classes for batches, on the CPU: the output kernel's numpy twin
against a per-row evaluation of its column program, the host path against the per-record
``predict_with_outputs``, the ``OutputPlan`` lowering under ``lowering_dry_run()`` against the
oracle's columns, and ``PredictionBatch`` carrying the outputs."""

import os
import pickle

import numpy as np
import pytest

from _output_cases import (bits, evaluate_rows, field, grid, probability_fields, program, raw_results,
                           top_k_reference, with_output)

from flink_jpmml_amd.api.batch import BatchOutputs, PredictionBatch, RecordBatch
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.bench import synth
from flink_jpmml_amd.ops import outputs as K
from flink_jpmml_amd.runtime.plans import NotLowerable, lowering_dry_run

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pmml")
IRIS_LO, IRIS_HI = [4.3, 2.0, 1.0, 0.1], [7.9, 4.4, 6.9, 2.5]


def iris_rows(n: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).uniform(IRIS_LO, IRIS_HI, (n, 4)).astype(np.float32)


# --------------------------------------------------------------------------- the kernel's twin


@pytest.mark.parametrize("m,C,n_col,k", grid())
def test_twin_equals_the_per_row_evaluation(m, C, n_col, k):
    score, valid, probs, aff = raw_results(m, C, seed=m + 7 * C + n_col)
    L = C if C else 5
    prog, tables = program(n_col, C, k, L, seed=n_col)
    label_table = np.append(np.where(np.arange(L) % 3 == 1, np.nan, np.arange(L) * 0.5), np.nan).astype(np.float32)
    if probs is not None:  # a view of a wider matrix: ldp > C
        wide = np.full((m, C + 3), 9.0, dtype=np.float32)
        wide[:, 1:1 + C] = probs
        probs = wide[:, 1:1 + C]
    for lt in (label_table, None):
        got = K.outputs_numpy(score, valid, prog, tables, probs=probs, affinity=aff, label_table=lt, k=k)
        want = evaluate_rows(score, valid, prog, tables, probs, aff, lt, k)
        for g, w, what in zip(got, want, ("out", "score", "valid")):
            assert np.array_equal(bits(g), bits(w)) if what != "valid" else np.array_equal(g, w), what


def test_twin_top_k_rule():
    """Entry r is the class of the r-th largest probability: ties to the lower class, NaN never
    selected, NaN past the non-NaN classes (k > C included) and on invalid rows."""
    p = np.array([[0.25, 0.5, 0.5, np.nan, 0.25],
                  [np.nan] * 5,
                  [0.0, 0.0, 1.0, 0.0, 0.0],
                  [0.2, 0.2, 0.2, 0.2, 0.2],
                  [0.1, -np.inf, np.nan, 0.3, 0.3]], dtype=np.float32)
    valid = np.array([1, 1, 1, 0, 1], dtype=np.uint8)
    score = np.zeros(5, dtype=np.float32)
    for k in (1, 3, 8):
        prog = np.array([(K.OP_TOPK_INDEX, r, 0, 0) for r in range(k)] + [(K.OP_TOPK_PROB, r, 0, 0) for r in range(k)],
                        dtype=np.int32)
        out, _, _ = K.outputs_numpy(score, valid, prog, np.zeros(1, np.float32), probs=p, k=k)
        for r in range(5):
            order = top_k_reference(p[r], k) if valid[r] else []
            want_i = np.array(order + [np.nan] * (k - len(order)), dtype=np.float32)
            want_p = np.array([p[r, c] for c in order] + [np.nan] * (k - len(order)), dtype=np.float32)
            assert np.array_equal(bits(out[r, :k]), bits(want_i)), (k, r)
            assert np.array_equal(bits(out[r, k:]), bits(want_p)), (k, r)
            # the host path's top-k is the same rule (a -inf probability ranks, a NaN never does)
            from flink_jpmml_amd.runtime.outputs import oracle_top_k

            hi, hp = oracle_top_k(p[r:r + 1], valid[r:r + 1] != 0, k)
            assert np.array_equal(np.where(hi[0] < 0, np.nan, hi[0]).astype(np.float32), want_i, equal_nan=True)
            assert np.array_equal(hp[0].astype(np.float32), want_p, equal_nan=True), (k, r)
    assert top_k_reference(p[0], 8) == [1, 2, 0, 4]
    assert top_k_reference(np.array([0.1, np.nan, -np.inf], dtype=np.float32), 3) == [0, 2]
    hi, hp = oracle_top_k(np.array([[0.1, np.nan, -np.inf]]), np.array([True]), 3)
    assert hi.tolist() == [[0, 2, -1]] and hp[0, 1] == -np.inf and np.isnan(hp[0, 2])
    # two classes, three ranks: a NaN tail
    out, _, _ = K.outputs_numpy(score[:1], valid[:1], np.array([(K.OP_TOPK_INDEX, 2, 0, 0)], dtype=np.int32),
                                np.zeros(1, np.float32), probs=p[:1, :2], k=3)
    assert np.isnan(out[0, 0])


def test_limits():
    assert K.rows_per_block(0, 1) == 256 and K.rows_per_block(256, 64) == 50
    for C, n_col in ((257, 1), (3, 65), (3, 0)):
        with pytest.raises(ValueError):
            K.rows_per_block(C, n_col)


# --------------------------------------------------------------------------- documents


def _forest(n_classes=3, string_label=False, n_trees=33, top=""):
    text = synth.random_forest_pmml(n_trees=n_trees, depth=4, n_features=8, n_classes=n_classes, seed=1)
    cats = [str(c) for c in range(n_classes)]
    label = field("label", "predictedValue", "string", "categorical") if string_label else \
        field("label", "predictedValue", "integer", "categorical")
    return with_output(text, label + probability_fields(cats) + field("p_win", "probability") + top)


def _gbdt_expr():
    expr = ('<Apply function="+"><Apply function="*"><FieldRef field="raw"/><Constant>2</Constant></Apply>'
            '<FieldRef field="f1"/></Apply>')
    flag = '<Apply function="greaterThan"><FieldRef field="twice"/><Constant>0.5</Constant></Apply>'
    return with_output(synth.gbdt_pmml(n_trees=12, depth=3, n_features=6, seed=4),
                       field("raw", "predictedValue") + field("twice", "transformedValue", inner=expr)
                       + field("flag", "decision", "boolean", "categorical", inner=flag))


def _kmeans_doc():
    with open(os.path.join(GOLDEN, "kmeans.xml")) as fh:
        return fh.read()


def _documents():
    """name -> (document, input matrix)."""
    X8 = synth.stream_matrix(70, 8, seed=2, missing_rate=0.02)
    km = _kmeans_doc()
    n_km = len(PmmlModel.from_string(km).active_fields)
    return {
        "iris": (synth.iris_logistic_pmml(), iris_rows(70)),
        "kmeans_golden": (km, np.abs(synth.stream_matrix(70, n_km, seed=3)) * 3),
        "gbdt_expression": (_gbdt_expr(), synth.stream_matrix(70, 6, seed=5, missing_rate=0.02)),
        "forest_string_label": (_forest(string_label=True), X8),
    }


DOCS = _documents()


@pytest.mark.parametrize("name", sorted(DOCS))
def test_host_path_equals_predict_with_outputs(name):
    text, X = DOCS[name]
    model = PmmlModel.from_string(text)
    compiled = model.compiled
    s, v, cols = compiled.outputs_matrix_oracle(X)
    s0, v0 = compiled.score_matrix_oracle(X)
    assert np.array_equal(v, v0) and np.array_equal(bits(s), bits(s0))
    assert list(cols) == compiled.output_fields and cols
    batch = RecordBatch(X)
    for i in range(len(X)):
        want = model.predict_with_outputs(batch.vector(i)).outputs
        got = {k: compiled.schema.decode(k, float(c[i])) for k, c in cols.items()}
        assert got == want, (i, got, want)
    # the public form: same columns, decoded through BatchOutputs
    s1, v1, outs = model.predict_batch_outputs(X)
    assert np.array_equal(v1, v) and outs.names == compiled.output_fields
    for k in outs.names:
        assert np.array_equal(outs[k], cols[k], equal_nan=True)
        assert outs.decode(k) == [model.predict_with_outputs(batch.vector(i)).outputs[k] for i in range(len(X))]


def test_rows_that_fail_preparation_hold_nan():
    text = synth.iris_logistic_pmml().replace('<MiningField name="sepal_width"/>',
                                              '<MiningField name="sepal_width" invalidValueTreatment="returnInvalid"/>')
    text = text.replace('<DataField name="sepal_width" optype="continuous" dataType="double"/>',
                        '<DataField name="sepal_width" optype="continuous" dataType="double">'
                        '<Interval closure="closedClosed" leftMargin="2" rightMargin="4.4"/></DataField>')
    X = iris_rows(9)
    X[4, 1] = 99.0
    s, v, cols = PmmlModel.from_string(text).compiled.outputs_matrix_oracle(X)
    for c in cols.values():
        assert np.isnan(c[4]) and not np.isnan(np.delete(c, 4)).any()


def test_iris_batch_outputs_has_probabilities_where_the_score_is_empty():
    """The capability no batch route had: a string-labelled classifier scores EmptyScore on every
    record (its label is no double), and its probability columns are there all the same."""
    model = PmmlModel.from_string(synth.iris_logistic_pmml())
    X = iris_rows(64)
    scores, valid, outs = model.predict_batch_outputs(X, top_k=2)
    assert not valid.any() and np.isnan(scores).all()
    assert outs.names == [f"probability(Iris-{c})" for c in ("setosa", "versicolor", "virginica")]
    assert outs.matrix.shape == (64, 3) and np.isfinite(outs.matrix).all()
    assert np.abs(outs.matrix.sum(axis=1) - 1.0).max() < 1e-12
    assert outs.categories == ["Iris-setosa", "Iris-versicolor", "Iris-virginica"]
    assert np.array_equal(outs.top_index[:, 0], outs.matrix.argmax(axis=1))
    assert np.array_equal(outs.top_probability[:, 0], outs.matrix.max(axis=1))
    # the streaming surface on the host scorer
    pb = model.predict_records(RecordBatch(X), outputs=True, top_k=2)
    assert not pb.valid.any() and np.array_equal(pb.outputs.matrix, outs.matrix)
    assert model.predict_records(RecordBatch(X)).outputs is None


# --------------------------------------------------------------------------- lowering (dry run)


def _classes_of(text):
    c = PmmlModel.from_string(text).compiled
    return c.evaluator.evaluate(c.columns(np.full((1, c.n_features), np.nan))).categories


def _classifier(text):
    cats = _classes_of(text)
    return with_output(text, field("label", "predictedValue", "string", "categorical") + probability_fields(cats)
                       + field("p_none", "probability", value="no-such-class") + field("p_win", "probability")
                       + field("w", "warning", "string", "categorical"))


def _linear_regression():
    fields = [f"f{j}" for j in range(5)]
    dd = "".join(f'<DataField name="{f}" optype="continuous" dataType="double"/>' for f in fields)
    ms = "".join(f'<MiningField name="{f}"/>' for f in fields)
    terms = "".join(f'<NumericPredictor name="{f}" coefficient="{0.25 * (j + 1) * (-1) ** j}"/>'
                    for j, f in enumerate(fields))
    return ('<PMML xmlns="http://www.dmg.org/PMML-4_3" version="4.3"><Header/>'
            f'<DataDictionary>{dd}<DataField name="y" optype="continuous" dataType="double"/></DataDictionary>'
            '<RegressionModel functionName="regression" modelName="lin">'
            f'<MiningSchema><MiningField name="y" usageType="target"/>{ms}</MiningSchema>'
            f'<Output>{field("value", "predictedValue")}{field("same", "transformedValue")}</Output>'
            f'<RegressionTable intercept="0.5">{terms}</RegressionTable></RegressionModel></PMML>')


def _double(label):
    try:
        return float(label)
    except (TypeError, ValueError):
        return float("nan")


def _mixed(n, F, seed):
    return synth.mixed_records(n, F, seed=seed, missing_rate=0.02)[1].astype(np.float32)


def _families():
    """name -> (document, inputs, plan options, top_k, the innermost plan class)."""
    X8 = synth.stream_matrix(70, 8, seed=2, missing_rate=0.02)
    X6 = synth.stream_matrix(70, 6, seed=5, missing_rate=0.02)
    km = with_output(synth.kmeans_pmml(n_clusters=5, n_features=4, seed=3),
                     field("id", "entityId", "string", "categorical") + field("cid", "clusterId", "integer", "categorical")
                     + field("label", "predictedValue", "string", "categorical") + field("aff", "affinity")
                     + field("caff", "clusterAffinity"))
    seg_values = field("value", "predictedValue") + field("same", "transformedValue")
    return {
        "linear_classification": (_classifier(synth.iris_logistic_pmml()), iris_rows(70), {}, 3, "LinearPlan"),
        "linear_regression": (_linear_regression(), synth.stream_matrix(70, 5, seed=1, missing_rate=0.02), {}, 0,
                              "LinearPlan"),
        "naive_bayes": (_classifier(synth.naive_bayes_pmml()), _mixed(70, 4, 6), {}, 2, "LinearPlan"),
        "glm_multinomial": (_classifier(synth.glm_pmml("multinomialLogistic")), _mixed(70, 3, 7), {}, 2, "LinearPlan"),
        "forest_votes": (_forest(), X8, {}, 3, "TreePlan"),
        "forest_16_classes": (_forest(16), X8, {}, 8, "TreePlan"),
        "gbdt_regression": (_gbdt_expr(), X6, {}, 0, "TreePlan"),
        "gbdt_binary_chain": (_classifier(synth.gbdt_pmml(n_trees=12, depth=3, n_features=6, seed=4,
                                                          objective="binary")), X6, {}, 2, "TreePlan"),
        "gbdt_multiclass_chain": (_classifier(synth.gbdt_pmml(n_trees=12, depth=3, n_features=6, seed=4,
                                                              objective="multiclass")), X6, {}, 2, "TreePlan"),
        "segmented_regression": (with_output(synth.segmented_pmml("selectFirst"), seg_values), X6, {}, 0,
                                 "SegmentedPlan"),
        "segmented_classification": (with_output(synth.segmented_pmml("majorityVote", classification=True),
                                                 field("label", "predictedValue", "string", "categorical")),
                                     X6, {}, 0, "SegmentedPlan"),
        "mlp_fused": (_classifier(synth.mlp_pmml(8, (16,), 3, seed=2, classification=True)), X8, {"mlp_impl": "fused"},
                      2, "MlpPlan"),
        "mlp_wide": (_classifier(synth.mlp_pmml(8, (16,), 3, seed=2, classification=True)), X8, {"mlp_impl": "wide"},
                     2, "WideMlpPlan"),
        "kmeans": (km, synth.stream_matrix(70, 4, seed=8, missing_rate=0.02), {}, 0, "ClusterPlan"),
        "kmeans_golden": DOCS["kmeans_golden"] + ({}, 0, "ClusterPlan"),
    }


FAMILIES = _families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_output_plan_lowers_and_matches_the_oracle(name):
    from flink_jpmml_amd.runtime.outputs import _base, oracle_top_k

    text, X, opts, top_k, plan_class = FAMILIES[name]
    compiled = PmmlModel.from_string(text).compiled
    with lowering_dry_run():
        plan = compiled.output_plan("cpu", top_k=top_k, **opts)
        assert compiled.output_plan("cpu", top_k=top_k, **opts) is plan  # cached like plan()
        assert type(_base(plan.inner)).__name__ == plan_class
        assert compiled.plan("cpu", **opts) is not plan.inner  # the scoring plan stays its own
        table = getattr(_base(compiled.plan("cpu", **opts)), "table", None)
        if table is not None:  # the scoring plan still decodes to the labels' doubles, not to indices
            want = np.array([_double(x) for x in plan.labels], dtype=np.float32)
            assert np.array_equal(bits(table.numpy()), bits(want)), name
            assert np.array_equal(bits(plan.label_table.numpy()[:-1]), bits(want)), name
        score, valid, wide = plan.score_outputs(X)
    s, v, cols = compiled.outputs_matrix_oracle(X)
    assert np.array_equal(valid.numpy(), v), name
    assert np.allclose(score.numpy(), s, rtol=1e-6, atol=0, equal_nan=True)
    assert plan.names == compiled.output_fields
    wide = wide.numpy()
    for j, k in enumerate(plan.names):
        # the raw results are the oracle's rounded to fp32; labels and encodings are exact
        if k == "twice":  # 2 * raw + f1 cancels: 2 * raw carries raw's rounding, the result its own
            bound = 2.0 ** -24 * (2 * np.abs(cols["raw"]) + np.abs(cols[k]))
            assert np.array_equal(np.isnan(wide[:, j]), np.isnan(cols[k]))
            assert np.all(np.nan_to_num(np.abs(wide[:, j] - cols[k])) <= np.nan_to_num(bound)), (name, k)
            continue
        assert np.allclose(wide[:, j], cols[k], rtol=3e-7, atol=1e-30, equal_nan=True), (name, k)
        if compiled.schema.is_string(k) or k in ("cid", "flag"):
            assert np.array_equal(wide[:, j], cols[k], equal_nan=True), (name, k)
    if top_k:
        res = compiled.result(X)
        P, ok = compiled.prepare(X)
        # the plan ranks the fp32 probabilities: compare on the oracle's rounded the same way
        ti, tp = oracle_top_k(np.asarray(res.probs, dtype=np.float32), res.valid & ok, top_k)
        outs = BatchOutputs.from_wide(plan.names, wide, top_k, compiled.schema, plan.categories)
        assert np.array_equal(outs.top_index, ti), name
        assert np.array_equal(bits(outs.top_probability), bits(tp.astype(np.float32))), name
        assert outs.categories == list(res.categories)


def _not_lowerable():
    km = synth.kmeans_pmml(n_clusters=5, n_features=4, seed=3)
    return {
        "reasonCode": (synth.scorecard_pmml(), "RC1", 0),
        "svm_probability": (with_output(synth.svm_pmml(n_features=4, n_sv=16), field("p1", "probability", value="1")),
                            "p1", 0),
        "knn_entity": (with_output(synth.knn_pmml(), field("nearest", "entityId", "string", "categorical")),
                       "nearest", 0),
        "named_entity_affinity": (with_output(km, field("a2", "entityAffinity", value="2")), "a2", 0),
        "rank_2": (with_output(synth.iris_logistic_pmml(), field("second", "predictedValue", "string", "categorical",
                                                                 rank=2)), "second", 0),
        "segmented_probability": (with_output(synth.segmented_pmml("majorityVote", classification=True),
                                              field("p0", "probability", value="0")), "p0", 0),
        "too_many_columns": (with_output(synth.iris_logistic_pmml(),
                                         "".join(field(f"c{i}", "predictedValue", "string", "categorical")
                                                 for i in range(65))), "65 columns", 0),
        "top_k_without_probabilities": (km, "top_k", 2),
    }


NOT_LOWERABLE = _not_lowerable()


@pytest.mark.parametrize("name", sorted(NOT_LOWERABLE))
def test_what_does_not_lower_names_the_field(name):
    text, needle, top_k = NOT_LOWERABLE[name]
    compiled = PmmlModel.from_string(text).compiled
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        compiled.output_plan("cpu", top_k=top_k)
    assert needle in str(e.value), str(e.value)


def test_top_k_out_of_range():
    compiled = PmmlModel.from_string(synth.iris_logistic_pmml()).compiled
    with lowering_dry_run(), pytest.raises(ValueError):
        compiled.output_plan("cpu", top_k=9)
    with pytest.raises(ValueError):
        PmmlModel.from_string(synth.iris_logistic_pmml()).predict_batch_outputs(iris_rows(3), top_k=9)


# --------------------------------------------------------------------------- PredictionBatch


def _prediction_batch(n=40, top_k=2):
    model = PmmlModel.from_string(_forest(string_label=True))
    X = synth.stream_matrix(n, 8, seed=9, missing_rate=0.02)
    return model, X, model.predict_records(RecordBatch(X), outputs=True, top_k=top_k)


def _same_outputs(a: BatchOutputs, b: BatchOutputs):
    assert a.names == b.names and a.categories == b.categories
    assert np.array_equal(a.matrix, b.matrix, equal_nan=True)
    assert np.array_equal(a.top_index, b.top_index)
    assert np.array_equal(a.top_probability, b.top_probability, equal_nan=True)


def test_prediction_batch_pickles_with_its_outputs():
    _, _, pb = _prediction_batch()
    back = pickle.loads(pickle.dumps(pb))
    assert np.array_equal(back.valid, pb.valid) and np.array_equal(back.scores, pb.scores, equal_nan=True)
    _same_outputs(back.outputs, pb.outputs)
    assert back.outputs.decode("label") == pb.outputs.decode("label")  # the vocabulary travels
    assert set(pb.outputs.decode("label")) <= {"0", "1", "2", None}
    plain = PredictionBatch.from_arrays(pb.scores, pb.valid)
    assert pickle.loads(pickle.dumps(plain)).outputs is None


def test_prediction_batch_concat_and_masked_keep_the_outputs():
    model, X, pb = _prediction_batch()
    parts = [model.predict_records(RecordBatch(X[a:b]), outputs=True, top_k=2) for a, b in ((0, 13), (13, 40))]
    whole = PredictionBatch.concat(parts)
    assert np.array_equal(whole.valid, pb.valid)
    _same_outputs(whole.outputs, pb.outputs)
    assert PredictionBatch.concat([parts[0], model.predict_records(RecordBatch(X[13:]))]).outputs is None
    with pytest.raises(ValueError):  # parts of different models / top_k do not concatenate
        BatchOutputs.concat([pb.outputs, model.predict_records(RecordBatch(X), outputs=True, top_k=1).outputs])
    ok = np.arange(40) % 3 != 0
    masked = pb.masked(ok)
    assert not masked.valid[~ok].any()
    assert np.isnan(masked.outputs.matrix[~ok]).all() and (masked.outputs.top_index[~ok] == -1).all()
    assert np.isnan(masked.outputs.top_probability[~ok]).all()
    assert np.array_equal(masked.outputs.matrix[ok], pb.outputs.matrix[ok], equal_nan=True)
    assert np.array_equal(masked.outputs.top_index[ok], pb.outputs.top_index[ok])
    assert pb.masked(None) is pb


def test_wrong_size_vectors_have_no_outputs():
    model = PmmlModel.from_string(synth.iris_logistic_pmml())
    from flink_jpmml_amd.api.vectors import DenseVector

    batch = RecordBatch.from_vectors([DenseVector([5.0, 3.0, 1.5, 0.2]), DenseVector([1.0, 2.0])], 4)
    pb = model.predict_records(batch, outputs=True)
    assert np.isfinite(pb.outputs.matrix[0]).all() and np.isnan(pb.outputs.matrix[1]).all()
