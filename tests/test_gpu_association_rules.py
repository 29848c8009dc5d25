"""Association rules on the GPU (``rules.hip``): every case of ``_rule_cases.py`` at the row counts
round the workgroup sizes, through ``OutputPlan.launch`` and ``predict_batch_outputs``; the direct
launch with guard elements on contiguous, wider-stride and misaligned inputs and on a side stream;
the record route under ``ScoringConfig(association_rules=True)``; a sparse batch. Everything is
compared on bit patterns and decoded strings with the independent reference: no tolerance."""

import numpy as np
import pytest
import torch

import _rule_cases as RC
from flink_jpmml_amd.api.batch import BatchOutputs, RecordBatch, SparseRecordBatch
from flink_jpmml_amd.api.pmml_model import PmmlModel

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in RC.CASES]
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)


def tiled(case, n):
    """``n`` rows cycling through the case's rows, and the reference row of each."""
    rows = np.arange(n) % len(case["X"])
    return np.ascontiguousarray(case["X"][rows]), rows


def same_outputs(outputs, a, b):
    """Two ``BatchOutputs`` of two separately loaded models: the numeric fields bit for bit, the string
    fields as decoded strings (each model's schema numbers the texts in the order it met them)."""
    assert a.names == b.names == [o["name"] for o in outputs]
    for j, o in enumerate(outputs):
        if RC.is_numeric(o):
            assert np.array_equal(RC.bits(np.asarray(a.matrix)[:, j]), RC.bits(np.asarray(b.matrix)[:, j])), o["name"]
        else:
            assert a.decode(o["name"]) == b.decode(o["name"]), o["name"]


@pytest.mark.parametrize("name", NAMES)
def test_every_case_at_every_size_through_the_plan(gpu, name):
    case = RC.CASE[name]
    cols, _ = RC.expected(name)
    model = RC.model(name)
    schema = model.compiled.schema
    plan = model.compiled.output_plan(gpu, association_rules=True)
    assert plan.rules is not None and plan.inner is None
    for n in SIZES:
        X, rows = tiled(case, n)
        Xd = torch.from_numpy(X).to(gpu)
        score, valid = plan.alloc_outputs(n)
        matrix = plan.alloc_matrix(n)
        plan.launch(Xd, score, valid, outputs=matrix)
        torch.cuda.synchronize(gpu)
        wide = matrix.cpu().numpy()
        assert np.isnan(score.cpu().numpy()).all() and not valid.cpu().numpy().any()
        assert RC.compare(case, cols, wide, BatchOutputs.from_wide(plan.names, wide, 0, schema).decode, rows) == [], \
            (name, n)
        s, v, outs = model.predict_batch_outputs(X, device=gpu, association_rules=True)
        assert np.isnan(s.cpu().numpy()).all() and not v.cpu().numpy().any()
        assert np.array_equal(RC.bits(outs.matrix.cpu().numpy()), RC.bits(wide)), (name, n)
        assert RC.compare(case, cols, outs.matrix.cpu().numpy(), outs.decode, rows) == [], (name, n)


@pytest.mark.parametrize("name", ["i31", "i65", "i129", "f128", "f64", "i1024"])
@pytest.mark.parametrize("layout", ["contiguous", "wide", "misaligned", "stream"])
def test_direct_launch_layouts_and_guards(gpu, name, layout):
    case = RC.CASE[name]
    _, plan = RC.dry_plan(name)
    T = plan.rules
    X, _ = tiled(case, 257)
    want = RC.twin(plan, X)  # sentinels where the kernel must not write: no such column here, guards apart
    prep = plan.prep.numpy() if plan.prep is not None else None
    stream = torch.cuda.Stream(gpu) if layout == "stream" else None
    got, rest = RC.launch_direct(T, X, prep, gpu, "contiguous" if layout == "stream" else layout, stream)
    assert np.array_equal(RC.bits(got), RC.bits(want)), (name, layout)
    assert (rest == RC.SENTINEL).all(), (name, layout)


def test_columns_of_other_fields_stay_untouched(gpu):
    """A matrix twice as wide as the rule columns: the kernel writes its own columns only."""
    case = RC.CASE["i33"]
    _, plan = RC.dry_plan("i33")
    T = plan.rules
    cols = T.cols.copy()
    cols[:, 3] *= 2  # every other column belongs to somebody else
    T2 = RC.retabled(T, cols=cols, width=2 * T.width)
    X, _ = tiled(case, 65)
    want = RC.twin(plan, X, T2)
    assert (want[:, 1::2] == RC.SENTINEL).all() and not (want[:, 0::2] == RC.SENTINEL).any()
    got, rest = RC.launch_direct(T2, X, plan.prep.numpy() if plan.prep is not None else None, gpu)
    assert np.array_equal(RC.bits(got), RC.bits(want))
    assert (rest == RC.SENTINEL).all()


@pytest.mark.parametrize("name", ["i65", "i129"])
def test_config_switch_serves_predict_records(gpu, name):
    from flink_jpmml_amd.config import ScoringConfig

    case = RC.CASE[name]
    cols, _ = RC.expected(name)
    model = PmmlModel.from_string(RC.document(case)).bind(
        gpu, ScoringConfig(device=gpu, association_rules=True, fallback="error"))
    assert model.scorer.kind == "null" and model.scorer.rule_plan is not None
    X, rows = tiled(case, 257)
    pb = model.predict_records(RecordBatch(X), outputs=True)
    assert not np.asarray(pb.valid, dtype=bool).any() and np.isnan(np.asarray(pb.scores)).all()
    host = PmmlModel.from_string(RC.document(case)).bind(None)
    hb = host.predict_records(RecordBatch(X), outputs=True)
    same_outputs(case["outputs"], pb.outputs, hb.outputs)
    assert RC.compare(case, cols, np.asarray(pb.outputs.matrix), pb.outputs.decode, rows) == []


def test_fallback_policy_of_a_document_the_kernel_cannot_take(gpu):
    from flink_jpmml_amd.api.exceptions import ModelLoadingException
    from flink_jpmml_amd.config import ScoringConfig

    text, field = RC.five_groups()
    with pytest.raises(ModelLoadingException) as e:
        PmmlModel.from_string(text).bind(gpu, ScoringConfig(device=gpu, association_rules=True, fallback="error"))
    assert repr(field) in str(e.value)
    model = PmmlModel.from_string(text).bind(gpu, ScoringConfig(device=gpu, association_rules=True, fallback="host"))
    assert model.scorer.rule_plan is None
    X = RC.CASE["i33"]["X"]
    pb = model.predict_records(RecordBatch(X), outputs=True)
    hb = PmmlModel.from_string(text).bind(None).predict_records(RecordBatch(X), outputs=True)
    same_outputs(RC.CASE["i33"]["outputs"] + [RC.out(field, "ruleId")], pb.outputs, hb.outputs)


@pytest.mark.parametrize("name", ["i65", "i129"])
def test_a_sparse_batch_equals_the_dense_one(gpu, name):
    case = RC.CASE[name]
    model = RC.model(name)
    plan = model.compiled.output_plan(gpu, association_rules=True)
    X, _ = tiled(case, 257)
    F = X.shape[1]
    vectors = []
    from flink_jpmml_amd import SparseVector

    for row in X:
        idx = [j for j in range(F) if not np.isnan(row[j])]
        vectors.append(SparseVector(F, idx, [float(row[j]) for j in idx]))
    batch = SparseRecordBatch.from_vectors(vectors, F)
    s, v, sparse = plan.score_csr_outputs(batch)
    ds, dv, dense = plan.score_outputs(X)
    torch.cuda.synchronize(gpu)
    assert np.array_equal(RC.bits(sparse.cpu().numpy()), RC.bits(dense.cpu().numpy()))
    assert np.isnan(s.cpu().numpy()).all() and not v.cpu().numpy().any()
    cols, _ = RC.expected(name)
    wide = sparse.cpu().numpy()
    rows = np.arange(257) % len(case["X"])
    assert RC.compare(case, cols, wide, BatchOutputs.from_wide(plan.names, wide, 0, model.compiled.schema).decode,
                      rows) == []
