"""``SparseRecordBatch`` (CSR record batches) on the host: construction, validation, the lazy
dense fallback, the numpy twin of the ``pmml_csr_expand`` kernel, and host scoring.

Yardstick: bit equality with ``pack_vectors`` / ``pack_vectors_masked`` cast to fp32."""

import numpy as np
import pytest

from _sparse_cases import FILLS, PAIRS, PATTERNS, bits, expected, make_csr, skewed_vectors


def _mixed_vectors():
    from flink_jpmml_amd import DenseVector, SparseVector

    nan = float("nan")
    return [
        DenseVector(1.0, 2.0, 3.0, 4.0),
        SparseVector(4, [3, 0], [0.5, -2.0]),  # unsorted on purpose: SparseVector sorts
        SparseVector(4, [], []),
        DenseVector(1.0, nan, 3.0, -0.0),  # a stored NaN
        DenseVector(1.0, 2.0),  # wrong size
        SparseVector(4, [1], [nan]),  # a stored NaN in a sparse vector
        SparseVector(7, [6], [1.0]),  # wrong size
        SparseVector(4, [0, 1, 2, 3], [4.0, 3.0, 2.0, 1.0]),
    ]


def _same_mask(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def test_to_csr_round_trip():
    from flink_jpmml_amd.api.vectors import to_csr

    vs = _mixed_vectors()
    indptr, idx, val = to_csr(vs, 4)
    assert indptr.dtype == np.int32 and idx.dtype == np.int32 and val.dtype == np.float32
    assert indptr.tolist() == [0, 4, 6, 6, 10, 10, 11, 11, 15]
    assert idx.tolist() == [0, 1, 2, 3, 0, 3, 0, 1, 2, 3, 1, 0, 1, 2, 3]
    want = np.array([1, 2, 3, 4, -2, .5, 1, np.nan, 3, -0.0, np.nan, 4, 3, 2, 1], dtype=np.float32)
    assert np.array_equal(bits(val), bits(want))
    e = to_csr([], 4)
    assert e[0].tolist() == [0] and e[1].size == 0 and e[2].size == 0


def test_from_vectors_matches_record_batch():
    from flink_jpmml_amd import SparseRecordBatch, SparseVector
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.utils.metrics import METRICS

    vs = _mixed_vectors()
    before = METRICS.counters["scoring.sparse_densified_host"]
    sb = SparseRecordBatch.from_vectors(vs, 4, model_id="m", payload=list(range(len(vs))), offset=5)
    assert isinstance(sb, RecordBatch)
    assert len(sb) == len(vs) and sb.n_features == 4 and sb.nnz == 15
    assert sb.model_id == "m" and sb.offset == 5 and list(sb.payload) == list(range(len(vs)))
    assert sb.size_ok().tolist() == [True, True, True, True, False, True, False, True]
    assert sb.vector(1) == SparseVector(4, [0, 3], [-2.0, 0.5])
    assert sb.vector(2) == SparseVector(4, [], [])
    assert sb.vector(-1) == SparseVector(4, [0, 1, 2, 3], [4.0, 3.0, 2.0, 1.0])
    v5 = sb.vector(5)
    assert v5.indices.tolist() == [1] and np.isnan(v5.data[0])
    with pytest.raises(IndexError):
        sb.vector(len(vs))
    assert METRICS.counters["scoring.sparse_densified_host"] == before  # nothing above densified

    dense = RecordBatch.from_vectors(vs, 4)
    rb = sb.to_record_batch()
    assert METRICS.counters["scoring.sparse_densified_host"] == before + 1
    assert type(rb) is RecordBatch and rb.model_id == "m" and rb.offset == 5
    assert np.array_equal(bits(rb.X), bits(dense.X))
    assert _same_mask(rb.absent, dense.absent)
    assert np.array_equal(rb.size_ok(), dense.size_ok())
    assert np.array_equal(bits(sb.X), bits(dense.X)) and sb.X.dtype == np.float32
    assert METRICS.counters["scoring.sparse_densified_host"] == before + 1  # cached


def test_all_dense_vectors_have_no_mask_like_record_batch():
    from flink_jpmml_amd import DenseVector, SparseRecordBatch
    from flink_jpmml_amd.api.batch import RecordBatch

    for vs in ([DenseVector(1.0, 2.0), DenseVector(3.0, 4.0)], [DenseVector(1.0, float("nan")), DenseVector(3.0, 4.0)]):
        rb, dense = SparseRecordBatch.from_vectors(vs, 2).to_record_batch(), RecordBatch.from_vectors(vs, 2)
        assert np.array_equal(bits(rb.X), bits(dense.X))
        assert _same_mask(rb.absent, dense.absent)
        assert rb.size_ok() is None and dense.size_ok() is None


BAD = {
    "indptr[0] != 0": ([1, 2], [0, 1], [1.0, 2.0]),
    "indptr decreasing": ([0, 2, 1, 2], [0, 1], [1.0, 2.0]),
    "indptr[-1] != nnz": ([0, 1], [0, 1], [1.0, 2.0]),
    "len(indices) != len(values)": ([0, 2], [0, 1], [1.0]),
    "index < 0": ([0, 1], [-1], [1.0]),
    "index >= width": ([0, 1], [3], [1.0]),
    "duplicate in a row": ([0, 2], [1, 1], [1.0, 2.0]),
    "descending in a row": ([0, 2], [1, 0], [1.0, 2.0]),
}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_validation_rules(rule):
    from flink_jpmml_amd import SparseRecordBatch

    indptr, idx, val = BAD[rule]
    with pytest.raises(ValueError):
        SparseRecordBatch(indptr, idx, val, 3)
    b = SparseRecordBatch(indptr, idx, val, 3, validated=True)  # skipped only when asked
    with pytest.raises(ValueError):
        b.validate()


def test_valid_edge_cases_and_model_ids():
    from flink_jpmml_amd import SparseRecordBatch

    # a row may restart at a lower column than the previous row's last; empty rows anywhere
    b = SparseRecordBatch(np.array([0, 0, 2, 2, 3, 3], dtype=np.int64), [1, 2, 0], [1.0, 2.0, 3.0], 3)
    assert len(b) == 5 and b.indptr.dtype == np.int64
    assert len(SparseRecordBatch([0], [], [], 3)) == 0
    with pytest.raises(ValueError, match="out of scope"):
        SparseRecordBatch([0, 1], [0], [1.0], 3, model_ids=["a"])
    with pytest.raises(ValueError):
        SparseRecordBatch([0, 1], [0], [1.0], 3, payload=[1, 2])


def test_from_csr_duck_type_and_pinned():
    from flink_jpmml_amd import SparseRecordBatch

    class Csr:  # what scipy.sparse.csr_matrix exposes
        indptr = np.array([0, 1, 3], dtype=np.int32)
        indices = np.array([2, 0, 1], dtype=np.int32)
        data = np.array([1.0, 2.0, 3.0], dtype=np.float64)
        shape = (2, 3)

    b = SparseRecordBatch.from_csr(Csr, model_id="x")
    assert b.width == 3 and b.values.dtype == np.float32 and b.model_id == "x"
    assert np.array_equal(bits(b.X), bits(np.array([[np.nan, np.nan, 1], [2, 3, np.nan]], dtype=np.float32)))
    assert SparseRecordBatch.from_csr(Csr, width=5).n_features == 5
    with pytest.raises(ValueError):
        SparseRecordBatch.from_csr(Csr, width=2)

    p = SparseRecordBatch.pinned(2, 8, 3)  # capacity above what is used
    assert len(p) == 2 and p.indices.size == 8 and p.values.size == 8
    p.indptr[:] = [0, 1, 3]
    p.indices[:3] = [2, 0, 1]
    p.values[:3] = [1.0, 2.0, 3.0]
    assert p.nnz == 3 and np.array_equal(bits(p.X), bits(b.X)) and np.array_equal(p.absent, b.absent)


@pytest.mark.parametrize("F,m", PAIRS)
def test_numpy_twin_equals_pack_vectors(F, m):
    from flink_jpmml_amd.ops.sparse import csr_expand_numpy

    for pattern in PATTERNS:
        csr = make_csr(F, m, pattern)
        want, absent = expected(*csr, F)
        for fill in FILLS:
            got = csr_expand_numpy(*csr, m, F, fill)
            ref = want["nan" if fill != fill else "fill"]
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(ref)), (pattern, fill)
        if pattern == "specials":  # a stored NaN survives the fill; an absent entry takes it
            got = csr_expand_numpy(*csr, m, F, -1.5)
            stored_nan = ~absent & np.isnan(want["nan"])
            assert stored_nan.any() and np.isnan(got[stored_nan]).all()
            assert (got[absent] == np.float32(-1.5)).all()


def test_numpy_twin_skips_out_of_range_entries():
    from flink_jpmml_amd.ops.sparse import csr_expand_numpy, rows_per_block

    # index >= width, a negative index, and an indptr that points past the entries: all skipped
    got = csr_expand_numpy(np.array([0, 2, 9]), np.array([1, 5, -1, 0], dtype=np.int32),
                           np.array([1, 2, 3, 4], dtype=np.float32), 2, 3, 0.0)
    assert got.tolist() == [[0, 1, 0], [4, 0, 0]]
    assert [rows_per_block(F) for F in (1, 64, 65, 257, 4096, 16384)] == [256, 256, 252, 63, 4, 1]
    with pytest.raises(ValueError):
        rows_per_block(16385)


def _gbdt_model():
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.bench.synth import gbdt_pmml

    return PmmlModel.from_string(gbdt_pmml(n_trees=12, depth=4, n_features=24, seed=7)), 24


def _kmeans_model(fixtures_dir):
    from flink_jpmml_amd.api.pmml_model import PmmlModel

    return PmmlModel.from_path(fixtures_dir["kmeans"]), 4


@pytest.mark.parametrize("which", ["kmeans", "gbdt"])
@pytest.mark.parametrize("replace_nan", [None, 0.0])
def test_host_predict_sparse_equals_dense_equals_per_record(which, replace_nan, fixtures_dir):
    from flink_jpmml_amd import SparseRecordBatch
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.utils.metrics import METRICS

    model, F = _kmeans_model(fixtures_dir) if which == "kmeans" else _gbdt_model()
    # fp32-exact values (CSR stores fp32), positive and in the k-means fixture's field ranges
    vs = skewed_vectors(64, F, seed=5, value_scale=1.0)
    if which == "kmeans":
        for v in vs:
            v.data[:] = np.abs(v.data) + 0.5
    before = METRICS.counters["scoring.sparse_densified_host"]
    sparse = model.predict(SparseRecordBatch.from_vectors(vs, F), replace_nan)
    assert METRICS.counters["scoring.sparse_densified_host"] == before + 1  # device=None: the dense fallback
    dense = model.predict(RecordBatch.from_vectors(vs, F), replace_nan)
    assert np.array_equal(sparse.valid, dense.valid)
    assert np.array_equal(bits(sparse.scores), bits(dense.scores))
    # per record: the same validity, and the float64 score rounded to the batch's fp32 exactly
    per_record = [model.predict(v, replace_nan).value for v in vs]
    assert [not t.is_empty for t in per_record] == sparse.valid.tolist()
    want = np.array([t.get_or_else(np.nan) for t in per_record], dtype=np.float64).astype(np.float32)
    assert np.array_equal(bits(sparse.scores), bits(want))
    assert model.predict_vectors(vs, replace_nan, sparse=True) == model.predict_vectors(vs, replace_nan)
    if replace_nan is not None:
        assert sparse.valid.any()


N1 = "a1b2c3d4-0000-4000-8000-000000000001"


def _kmeans_chunks():
    """Three chunks of fp32-exact vectors in the k-means fixture's field ranges."""
    chunks = [skewed_vectors(n, 4, seed=70 + n) for n in (40, 3, 25)]
    for vs in chunks:
        for v in vs:
            v.data[:] = np.abs(v.data) + 0.5
    return chunks


def _columns(preds):
    return (np.concatenate([bits(p.scores) for p in preds]), np.concatenate([p.valid for p in preds]))


@pytest.mark.parametrize("batch_size", [None, 16])
def test_quick_evaluate_and_evaluate_accept_sparse_batches(batch_size, fixtures_dir):
    """Sparse batches are batches to every operator path, with the per-record micro-batcher
    (``batch_size``) on or off: the same results as the dense stream, each batch counted by its
    rows, never taken for a per-record event."""
    from flink_jpmml_amd import ModelReader, SparseRecordBatch
    from flink_jpmml_amd.api.batch import PredictionBatch, RecordBatch
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.stream import StreamExecutionEnvironment
    from flink_jpmml_amd.utils.metrics import METRICS

    chunks = _kmeans_chunks()
    reader = ModelReader(fixtures_dir["kmeans"])
    cfg = ScoringConfig(device=None, batch_size=batch_size)

    def quick(make):
        env = StreamExecutionEnvironment(config=cfg)
        out = env.from_batches([make(vs, 4) for vs in chunks]).quick_evaluate(reader).collect()
        assert [type(p) for p, _ in out] == [PredictionBatch] * 3
        assert [len(b) for _, b in out] == [40, 3, 25]
        return _columns([p for p, _ in out])

    def evaluate(make):
        env = StreamExecutionEnvironment(config=cfg)
        out = env.from_batches([make(vs, 4) for vs in chunks]).evaluate(
            reader, lambda b, m: (len(b), m.predict(b, 0.0))).collect()
        assert [n for n, _ in out] == [40, 3, 25]
        return _columns([p for _, p in out])

    for run in (quick, evaluate):
        rows0 = METRICS.counters["job.records_in"]
        s, v = run(SparseRecordBatch.from_vectors)
        assert METRICS.counters["job.records_in"] - rows0 == 68
        sd, vd = run(RecordBatch.from_vectors)
        assert np.array_equal(v, vd) and np.array_equal(s, sd) and v.any()


@pytest.mark.parametrize("batch_size", [None, 16])
def test_connected_stream_accepts_sparse_batches_with_one_model_id(batch_size, fixtures_dir):
    from flink_jpmml_amd import AddMessage, SparseRecordBatch
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.stream import StreamExecutionEnvironment

    chunks = _kmeans_chunks()

    def run(make):
        seq = [("R", AddMessage(N1, 1, fixtures_dir["kmeans"], 0))] + \
              [("L", make(vs, 4, model_id=f"{N1}_1")) for vs in chunks]
        env = StreamExecutionEnvironment(config=ScoringConfig(device=None, batch_size=batch_size))
        ev, ctrl = env.from_either(seq)
        out = ev.with_support_stream(ctrl).evaluate(lambda b, m: (b.model_id, len(b), m.predict(b))).collect()
        assert [(mid, n) for mid, n, _ in out] == [(f"{N1}_1", n) for n in (40, 3, 25)]
        return _columns([p for _, _, p in out])

    s, v = run(SparseRecordBatch.from_vectors)
    sd, vd = run(RecordBatch.from_vectors)
    assert np.array_equal(v, vd) and np.array_equal(s, sd) and v.any()
    qs = StreamExecutionEnvironment(config=ScoringConfig(device=None, batch_size=batch_size))
    ev, ctrl = qs.from_either([("R", AddMessage(N1, 1, fixtures_dir["kmeans"], 0))] + [
        ("L", SparseRecordBatch.from_vectors(vs, 4, model_id=f"{N1}_1")) for vs in chunks])
    out = ev.with_support_stream(ctrl).quick_evaluate().collect()
    sq, vq = _columns([p for p, _ in out])
    assert np.array_equal(vq, vd) and np.array_equal(sq, sd)


def test_model_ids_cannot_be_set_after_construction():
    from flink_jpmml_amd import SparseRecordBatch

    b = SparseRecordBatch([0, 1, 1], [0], [1.0], 3)
    with pytest.raises(ValueError, match="out of scope"):
        b.model_ids = ["a", "b"]
    b.model_ids = None
    assert b.model_ids is None and not b.has_model_ids and b.split_by_model() == [b]
    assert b.row_index is None and b.ready is None and b.created > 0  # the base initialiser ran
