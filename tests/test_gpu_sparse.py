"""CSR record batches on the MI355X: the ``pmml_csr_expand`` kernel against the host
densification (``pack_vectors`` / ``pack_vectors_masked`` cast to fp32) bit for bit, and sparse
batches through the H2D ring, the synchronous plan path and the DSL against their dense
counterparts, exactly — the kernel only moves bits, so nothing here has a tolerance."""

import numpy as np
import pytest

from _sparse_cases import FILLS, PAIRS, PATTERNS, bits, expected, make_csr, skewed_vectors

pytestmark = pytest.mark.gpu


def _expand(gpu, csr, m, F, fill):
    import torch

    from flink_jpmml_amd.ops.sparse import csr_expand

    indptr, idx, val = (torch.from_numpy(a).to(gpu) for a in csr)
    out = torch.empty((m, F), dtype=torch.float32, device=gpu)
    csr_expand(indptr, idx, val, out, int(csr[0][-1]), fill)
    return out.cpu().numpy()


def test_rows_per_block_matches_the_library(gpu):
    from flink_jpmml_amd.ops import _lib
    from flink_jpmml_amd.ops.sparse import rows_per_block

    lib = _lib.load()
    for F in sorted({F for F, _ in PAIRS} | {2, 63, 65, 512, 8191, 16383}):
        assert lib.pmml_csr_expand_rows(F) == rows_per_block(F)
    assert lib.pmml_csr_expand_rows(0) == 0 and lib.pmml_csr_expand_rows(16385) == 0


@pytest.mark.parametrize("F,m", PAIRS)
def test_expand_kernel_equals_pack_vectors(gpu, F, m):
    for pattern in PATTERNS:
        csr = make_csr(F, m, pattern)
        want, absent = expected(*csr, F)
        for fill in FILLS:
            got = _expand(gpu, csr, m, F, fill)
            ref = want["nan" if fill != fill else "fill"]
            assert np.array_equal(bits(got), bits(ref)), (pattern, fill)
        if pattern == "specials":  # a stored NaN survives the fill; an absent entry takes it
            got = _expand(gpu, csr, m, F, -1.5)
            stored_nan = ~absent & np.isnan(want["nan"])
            assert stored_nan.any() and np.isnan(got[stored_nan]).all()
            assert (got[absent] == np.float32(-1.5)).all()


def test_expand_kernel_offset_output_takes_the_4_byte_path(gpu):
    """An output whose base is 4 bytes off a 16-byte boundary (a row view of a wider buffer)."""
    import torch

    from flink_jpmml_amd.ops.sparse import csr_expand

    F, m = 64, 300
    csr = make_csr(F, m, "random5", seed=3)
    want, _ = expected(*csr, F)
    buf = torch.full((m * F + 2,), 7.0, dtype=torch.float32, device=gpu)
    out = buf[1:1 + m * F].view(m, F)
    assert out.data_ptr() % 16 == 4
    csr_expand(*(torch.from_numpy(a).to(gpu) for a in csr), out, int(csr[0][-1]))
    assert np.array_equal(bits(out.cpu().numpy()), bits(want["nan"]))
    assert buf[0].item() == 7.0 and buf[-1].item() == 7.0  # nothing outside the tile


def _linear_pmml(n_features: int) -> str:
    """A plain linear ``RegressionModel`` over ``n_features`` continuous fields."""
    fields = [f"f{j}" for j in range(n_features)]
    dd = "".join(f'<DataField name="{f}" optype="continuous" dataType="double"/>' for f in fields)
    ms = "".join(f'<MiningField name="{f}"/>' for f in fields)
    terms = "".join(f'<NumericPredictor name="{f}" coefficient="{0.25 * (j + 1) * (-1) ** j}"/>'
                    for j, f in enumerate(fields))
    return (f'<PMML xmlns="http://www.dmg.org/PMML-4_3" version="4.3"><Header/>'
            f'<DataDictionary>{dd}<DataField name="y" optype="continuous" dataType="double"/></DataDictionary>'
            f'<RegressionModel functionName="regression" modelName="lin">'
            f'<MiningSchema><MiningField name="y" usageType="target"/>{ms}</MiningSchema>'
            f'<RegressionTable intercept="0.5">{terms}</RegressionTable></RegressionModel></PMML>')


def _models():
    from flink_jpmml_amd.bench.synth import gbdt_pmml, kmeans_pmml

    return {
        "gbdt": (gbdt_pmml(n_trees=20, depth=4, n_features=96, seed=11), 96),
        "kmeans": (kmeans_pmml(n_clusters=8, n_features=32, seed=3), 32),
        "regression": (_linear_pmml(7), 7),
    }


@pytest.fixture(scope="module")
def bound(gpu):
    """``name -> (PmmlModel bound to the GPU with micro_batch=256, width)``, lowered once."""
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.config import ScoringConfig

    out = {}
    models = _models()
    models["gbdt_auto"] = models["gbdt"]
    for name, (text, F) in models.items():
        # auto lowering gives this small GBDT to the wide perfect kernel ("gbdt_auto", what users
        # get); "gbdt" asks for the pointer walk
        opts = {"layout": "pointer"} if name == "gbdt" else {}
        cfg = ScoringConfig(device=gpu, micro_batch=256, pipeline_depth=3, fallback="error", plan_opts=opts)
        model = PmmlModel.from_string(text).bind(gpu, cfg)
        assert model.on_device
        out[name] = (model, F)
    return out


def _counters():
    from flink_jpmml_amd.utils.metrics import METRICS

    c = METRICS.counters
    return c["scoring.rows_sparse_device"], c["scoring.sparse_densified_host"], c["scoring.h2d_bytes_sparse"]


def _same(a, b):
    assert np.array_equal(a.valid, b.valid)
    assert np.array_equal(bits(a.scores), bits(b.scores))


def test_gbdt_takes_the_pointer_path(bound):
    plan = bound["gbdt"][0].scorer.plan
    assert getattr(plan, "layout", None) == "pointer", getattr(plan, "layout", None)
    assert bound["gbdt_auto"][0].scorer.plan.layout == "perfect"


@pytest.mark.parametrize("name", ["gbdt", "gbdt_auto", "kmeans", "regression"])
@pytest.mark.parametrize("replace_nan", [None, 0.0])
def test_predict_sparse_equals_dense_and_oracle_validity(bound, name, replace_nan):
    from flink_jpmml_amd import SparseRecordBatch
    from flink_jpmml_amd.api.batch import RecordBatch

    model, F = bound[name]
    vs = skewed_vectors(1000, F, seed=17)
    dense_batch = RecordBatch.from_vectors(vs, F)
    dense = model.predict(dense_batch, replace_nan)
    rows0, dens0, bytes0 = _counters()
    sb = SparseRecordBatch.from_vectors(vs, F)
    sparse = model.predict(sb, replace_nan)
    _same(sparse, dense)
    rows1, dens1, bytes1 = _counters()
    assert rows1 - rows0 == 1000 and dens1 == dens0
    assert bytes1 - bytes0 == 4 * (1000 + 4) + 8 * sb.nnz  # 4 slices of micro_batch = 256
    _, vref = model.compiled.score_matrix_oracle(dense_batch.X, replace_nan, dense_batch.absent)
    assert np.array_equal(sparse.valid, vref)
    assert sparse.valid.any()


def test_slices_start_mid_array(gpu, bound):
    """micro_batch = 256 over 1000 skewed rows: four slices, three starting mid-array, against
    the same batch in one slice."""
    from flink_jpmml_amd import SparseRecordBatch
    from flink_jpmml_amd.runtime.engine import StreamingScorer

    model, F = bound["gbdt"]
    sb = SparseRecordBatch.from_vectors(skewed_vectors(1000, F, seed=23), F)
    one = StreamingScorer(model.scorer.plan, micro_batch=1024, depth=2)
    for replace_nan in (None, 0.25):
        _same(model.scorer.submit_batch(sb, replace_nan), one.submit_batch(sb, replace_nan))
    one.drain()


def test_ring_reuse_growth_and_dense_interleave(gpu, bound):
    """3 x depth + 1 sparse batches of different nnz through one scorer without waiting in
    between, then a dense batch, then a sparse one: staging growth and slot hazards."""
    from flink_jpmml_amd import SparseRecordBatch
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.runtime.engine import StreamingScorer

    model, F = bound["kmeans"]
    scorer = StreamingScorer(model.scorer.plan, micro_batch=256, depth=3, max_inflight=16)
    sizes = [40, 700, 130, 256, 1000, 3, 513, 257, 90, 768]  # 3 * depth + 1
    batches = [skewed_vectors(n, F, seed=100 + i) for i, n in enumerate(sizes)]
    futures = [scorer.submit_batch(SparseRecordBatch.from_vectors(vs, F)) for vs in batches]
    dense_vs = skewed_vectors(600, F, seed=200)
    futures.append(scorer.submit_batch(RecordBatch.from_vectors(dense_vs, F)))
    last = skewed_vectors(777, F, seed=201)
    futures.append(scorer.submit_batch(SparseRecordBatch.from_vectors(last, F), 0.0))
    want = [model.predict(RecordBatch.from_vectors(vs, F)) for vs in batches + [dense_vs]]
    want.append(model.predict(RecordBatch.from_vectors(last, F), 0.0))
    for got, ref in zip(futures, want):
        _same(got, ref)
    scorer.drain()


def test_pageable_and_pinned_batches(bound):
    from flink_jpmml_amd import SparseRecordBatch
    from flink_jpmml_amd.api.batch import RecordBatch

    model, F = bound["regression"]
    vs = skewed_vectors(700, F, seed=31)
    dense = model.predict(RecordBatch.from_vectors(vs, F))
    pageable = SparseRecordBatch.from_vectors(vs, F)
    assert pageable._pinned is None
    _same(model.predict(pageable), dense)
    p = SparseRecordBatch.pinned(len(vs), pageable.nnz + 50, F)  # filled in place, capacity to spare
    assert p._pinned is not None and all(t.is_pinned() for t in p._pinned)
    p.indptr[:] = pageable.indptr
    p.indices[:pageable.nnz] = pageable.indices
    p.values[:pageable.nnz] = pageable.values
    _same(model.predict(p), dense)
    tp = pageable.to_pinned()
    assert tp._pinned is not None and tp.to_pinned() is tp
    _same(model.predict(tp), dense)


@pytest.mark.parametrize("replace_nan", [None, 0.0])
def test_predict_vectors_sparse_flag(gpu, bound, replace_nan):
    from flink_jpmml_amd import DenseVector

    model, F = bound["kmeans"]
    vs = skewed_vectors(300, F, seed=41) + [DenseVector(np.arange(F) / 8.0), DenseVector(1.0, 2.0)]
    rows0, dens0, _ = _counters()
    sparse = model.predict_vectors(vs, replace_nan, device=gpu, sparse=True)
    assert _counters()[1] == dens0
    assert sparse == model.predict_vectors(vs, replace_nan, device=gpu, sparse=False)
    assert sparse[-1].value.is_empty  # the wrong-size vector


def test_quick_evaluate_accepts_sparse_batches(gpu, tmp_path):
    from flink_jpmml_amd import ModelReader, SparseRecordBatch
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.stream import StreamExecutionEnvironment

    text, F = _models()["kmeans"]
    path = tmp_path / "kmeans.pmml"
    path.write_text(text)
    chunks = [skewed_vectors(n, F, seed=50 + n) for n in (300, 10, 500)]
    cfg = ScoringConfig(device=gpu, micro_batch=256, fallback="error")

    def run(make):
        env = StreamExecutionEnvironment(config=cfg)
        out = env.from_batches([make(vs, F) for vs in chunks]).quick_evaluate(ModelReader(str(path))).collect()
        return (np.concatenate([p.scores for p, _ in out]), np.concatenate([p.valid for p, _ in out]))

    rows0, dens0, _ = _counters()
    s, v = run(SparseRecordBatch.from_vectors)
    rows1, dens1, _ = _counters()
    assert rows1 - rows0 == 810 and dens1 == dens0
    sd, vd = run(RecordBatch.from_vectors)
    assert np.array_equal(v, vd) and np.array_equal(bits(s), bits(sd))
