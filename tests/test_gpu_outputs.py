"""PMML Output fields and top-k classes on the MI355X: ``pmml_outputs_launch`` against its numpy
twin bit for bit, every required family through its ``OutputPlan`` against the scoring plan, the
index-mode plan and the float64 oracle, the streaming routes against the synchronous one, and the
fallback policy."""

import numpy as np
import pytest

from _output_cases import bits, field, grid, program, raw_results, with_output
from test_batch_outputs import FAMILIES, iris_rows

pytestmark = pytest.mark.gpu

GUARD = 7.0


def _launch(gpu, score, valid, prog, tables, probs, aff, label_table, k, ldo_pad=0, ldp_pad=0, offset=0):
    """The kernel over host arrays; ``out`` sits in a guarded buffer (``offset`` floats in, rows
    ``ldo_pad`` floats apart), ``probs`` optionally as a column view of a wider matrix."""
    import torch

    from flink_jpmml_amd.ops.outputs import outputs_launch

    m, n_col = len(score), len(prog)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    ldo = n_col + ldo_pad
    buf = torch.full((offset + m * ldo + 4,), GUARD, dtype=torch.float32, device=gpu)
    out = buf[offset: offset + m * ldo].view(m, ldo)[:, :n_col]
    pt = None
    if probs is not None:
        C = probs.shape[1]
        wide = torch.full((m, C + ldp_pad), GUARD, dtype=torch.float32, device=gpu)
        wide[:, :C] = t(probs)
        pt = wide[:, :C]
    so = torch.full((m + 2,), GUARD, dtype=torch.float32, device=gpu)
    vo = torch.full((m + 2,), 9, dtype=torch.uint8, device=gpu)
    outputs_launch(t(score), t(valid), out, t(prog), t(tables), probs=pt, affinity=t(aff), label_table=t(label_table),
                   k=k, score_out=so[1:m + 1], valid_out=vo[1:m + 1])
    torch.cuda.synchronize()
    return out.cpu().numpy(), so.cpu().numpy(), vo.cpu().numpy(), buf.cpu().numpy(), out.data_ptr()


def _check(gpu, m, C, n_col, k, **layout):
    from flink_jpmml_amd.ops.outputs import outputs_numpy

    score, valid, probs, aff = raw_results(m, C, seed=m + 7 * C + n_col)
    L = C if C else 5
    prog, tables = program(n_col, C, k, L, seed=n_col)
    lt = np.append(np.where(np.arange(L) % 3 == 1, np.nan, np.arange(L) * 0.5), np.nan).astype(np.float32)
    for label_table in (lt, None):
        want, ws, wv = outputs_numpy(score, valid, prog, tables, probs=probs, affinity=aff, label_table=label_table, k=k)
        out, so, vo, buf, ptr = _launch(gpu, score, valid, prog, tables, probs, aff, label_table, k, **layout)
        assert np.array_equal(bits(out), bits(want)), (m, C, n_col, k, layout)
        assert np.array_equal(bits(so[1:-1]), bits(ws)) and np.array_equal(vo[1:-1], wv)
        # guard words: in front of out, between its rows, behind it, and around score / valid
        off, pad = layout.get("offset", 0), layout.get("ldo_pad", 0)
        body = buf[off: off + m * (n_col + pad)].reshape(m, n_col + pad)
        assert (buf[:off] == GUARD).all() and (buf[off + m * (n_col + pad):] == GUARD).all()
        assert (body[:, n_col:] == GUARD).all()
        assert so[0] == GUARD and so[-1] == GUARD and vo[0] == 9 and vo[-1] == 9
    return ptr


def test_rows_per_block_matches_the_library(gpu):
    from flink_jpmml_amd.ops import _lib
    from flink_jpmml_amd.ops.outputs import rows_per_block

    lib = _lib.load()
    for C in (0, 1, 2, 3, 16, 17, 64, 255, 256):
        for n_col in (1, 2, 3, 8, 33, 63, 64):
            assert lib.pmml_outputs_rows(C, n_col) == rows_per_block(C, n_col)
    assert lib.pmml_outputs_rows(257, 1) == 0 and lib.pmml_outputs_rows(3, 65) == 0 and lib.pmml_outputs_rows(3, 0) == 0


@pytest.mark.parametrize("m,C,n_col,k", grid())
def test_kernel_equals_the_twin(gpu, m, C, n_col, k):
    _check(gpu, m, C, n_col, k)  # contiguous, 16-byte aligned: the float4 paths
    _check(gpu, m, C, n_col, k, ldo_pad=3, ldp_pad=5)  # ldo > n_col, a probs view of a wider matrix


def test_kernel_offset_output_takes_the_4_byte_path(gpu):
    """An ``out`` base 4 bytes off a 16-byte boundary."""
    for m, C, n_col, k in ((257, 16, 8, 3), (65, 3, 3, 1), (300, 0, 4, 0)):
        ptr = _check(gpu, m, C, n_col, k, offset=1)
        assert ptr % 16 == 4


# --------------------------------------------------------------------------- families

ROWS = (1, 65, 257, 4097)

# |device - float64 oracle| the family's own GPU test allows for the same quantity
TOLERANCE = {
    "LinearPlan": 2e-5,      # tests/test_gpu_svm_lr.py: iris logistic probabilities, atol=2e-5
    "TreePlan": 1e-4,        # __graft_entry__.smoke(): GBDT sums, 1e-4 (vote fractions are far inside)
    "SegmentedPlan": 1e-5,   # tests/test_gpu_segmented.py: rtol = atol = 1e-5
    "MlpPlan": 1e-3,         # tests/test_gpu_mlp.py: 1e-3 * scale, probabilities have scale 1
    "WideMlpPlan": 1e-3,
    "ClusterPlan": 2e-5,     # tests/test_gpu_kernels.py: fp32 sums, rtol = atol = 2e-5
}
GAP = 1e-4


# The compared ranks of a row must be tied exactly or at least GAP apart in the oracle; at most 1 % of
# the rows may fall out for that. The lower ranks of the iris softmax are the exception: two classes
# that are both improbable (p < 1e-4) are closer than GAP on most rows however well they are
# computed, so its ranks 2 and 3 are compared on the rows the rule keeps, without the 1 % cap. Its
# winner, and every rank of every other classifier, keep the cap.
UNCAPPED_LOWER_RANKS = {"linear_classification"}


def _inputs(name, n):
    X = FAMILIES[name][1]
    F = X.shape[1]
    rng = np.random.default_rng(n)
    if name == "linear_classification":  # uniform over the iris box: default_rng(0), 2 % missing
        Y = iris_rows(n, seed=0)
        Y[rng.random(Y.shape) < 0.02] = np.nan
        return Y
    rows = rng.integers(0, len(X), n)
    Y = X[rows].copy()
    # fresh values around the fixture's rows, 2 % of them missing (categorical codes stay codes)
    if name in ("naive_bayes", "glm_multinomial"):
        Y[:, :-1] += rng.standard_normal((n, F - 1)).astype(np.float32) * 0.5
    else:
        Y += rng.standard_normal((n, F)).astype(np.float32) * 0.5
        if name in ("linear_classification", "kmeans_golden"):
            Y = np.abs(Y)
    Y[rng.random(Y.shape) < 0.02] = np.nan
    return np.ascontiguousarray(Y, dtype=np.float32)


@pytest.fixture(scope="module")
def lowered(gpu):
    """name -> (compiled, output plan, scoring plan), each lowered once."""
    from flink_jpmml_amd.api.pmml_model import PmmlModel

    out = {}
    for name, (text, _, opts, top_k, _) in FAMILIES.items():
        compiled = PmmlModel.from_string(text).compiled
        out[name] = (compiled, compiled.output_plan(gpu, top_k=top_k, **opts), compiled.plan(gpu, **opts))
    return out


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_outputs(gpu, lowered, name):
    import torch

    from flink_jpmml_amd.api.batch import BatchOutputs
    from flink_jpmml_amd.runtime.outputs import _base, oracle_top_k

    compiled, plan, scoring = lowered[name]
    plan_class = FAMILIES[name][4]
    assert type(_base(plan.inner)).__name__ == plan_class and plan.inner is not scoring
    tol = TOLERANCE[plan_class]
    for n in ROWS:
        X = _inputs(name, n)
        s, v, wide = plan.score_outputs(X)
        s0, v0 = scoring.score(X)
        torch.cuda.synchronize()
        # (a) the reference score is the scoring plan's, bit for bit
        assert np.array_equal(v.cpu().numpy(), v0.cpu().numpy()), (name, n)
        assert np.array_equal(bits(s.cpu().numpy()), bits(s0.cpu().numpy())), (name, n)
        wide = wide.cpu().numpy()
        outs = BatchOutputs.from_wide(plan.names, wide, plan.top_k, compiled.schema, plan.categories)
        # (b) probability / affinity columns are the index-mode plan's own bits
        Xt = torch.from_numpy(X).to(gpu)
        rs = torch.empty(n, dtype=torch.float32, device=gpu)
        rv = torch.empty(n, dtype=torch.uint8, device=gpu)
        kw = {}
        if plan.C:
            kw["probs"] = torch.full((n, plan.C), np.nan, dtype=torch.float32, device=gpu)
        if plan._affinity:
            kw["affinity"] = torch.full((n,), np.nan, dtype=torch.float32, device=gpu)
        plan.inner.launch(Xt, rs, rv, **kw)
        torch.cuda.synchronize()
        raw_ok = rv.cpu().numpy() != 0
        for j, (op, arg, _, _) in enumerate(plan.prog_np[: plan.n_named]):
            col = wide[:, plan.kernel_dst[j]]
            if op == 2:  # PROB
                want = np.where(raw_ok, kw["probs"].cpu().numpy()[:, arg], np.float32(np.nan))
                assert np.array_equal(bits(col), bits(want)), (name, n, plan.names[plan.kernel_dst[j]])
            elif op == 4:  # AFFINITY
                want = np.where(raw_ok, kw["affinity"].cpu().numpy(), np.float32(np.nan))
                assert np.array_equal(bits(col), bits(want)), (name, n)
        # (c) the float64 oracle
        so, vo, cols = compiled.outputs_matrix_oracle(X)
        assert np.array_equal(v.cpu().numpy(), vo), (name, n)
        res = compiled.result(X)
        _, ok = compiled.prepare(X)
        probs64 = None if res.probs is None else np.asarray(res.probs, dtype=np.float64)
        k = max(1, plan.top_k)
        rank_sure = [np.ones(n, dtype=bool) for _ in range(k)]  # rows on which rank r is decided
        if probs64 is not None:
            srt = -np.sort(-np.nan_to_num(probs64, nan=-np.inf), axis=1)[:, : k + 1]
            with np.errstate(invalid="ignore"):  # NaN probabilities rank last on both sides
                gaps = srt[:, :-1] - srt[:, 1:]
            unsafe = (gaps > 0) & (gaps < GAP)  # [n, g]: between rank g and rank g + 1
            for r in range(k):
                for g in (r - 1, r):
                    if 0 <= g < unsafe.shape[1]:
                        rank_sure[r] &= ~unsafe[:, g]
                if r == 0 or name not in UNCAPPED_LOWER_RANKS:
                    assert (~rank_sure[r]).mean() <= 0.01, (name, n, r, (~rank_sure[r]).mean())
        sure = rank_sure[0]  # the winner: labels and its probability
        for j, nm in enumerate(plan.names):
            got, want = wide[:, j].astype(np.float64), cols[nm]
            exact = compiled.schema.is_string(nm) or nm in ("cid", "flag")
            rows = sure if exact else np.ones(n, dtype=bool)
            assert np.array_equal(np.isnan(got[rows]), np.isnan(want[rows])), (name, n, nm)
            if exact:
                assert np.array_equal(got[rows], want[rows], equal_nan=True), (name, n, nm)
            elif nm == "p_win":  # the winner's probability: the winner may differ inside a gap
                assert np.nanmax(np.abs(got[sure] - want[sure]), initial=0.0) <= tol, (name, n, nm)
            elif nm == "twice":  # 2 * raw + f1: twice the value's tolerance
                assert np.nanmax(np.abs(got - want), initial=0.0) <= 2 * tol, (name, n, nm)
            elif plan_class in ("ClusterPlan", "SegmentedPlan"):
                # per element, as the tests named above do it: rtol = atol = tol
                np.testing.assert_allclose(got, want, rtol=tol, atol=tol, equal_nan=True, err_msg=str((name, n, nm)))
            else:
                assert np.nanmax(np.abs(got - want), initial=0.0) <= tol, (name, n, nm)
        if plan.top_k:
            ti, tp = oracle_top_k(probs64, res.valid & ok, plan.top_k)
            for r in range(plan.top_k):
                rows = rank_sure[r]
                assert np.array_equal(outs.top_index[rows, r], ti[rows, r]), (name, n, r)
                assert np.array_equal(np.isnan(outs.top_probability[rows, r]), np.isnan(tp[rows, r])), (name, n, r)
                assert np.nanmax(np.abs(outs.top_probability[rows, r] - tp[rows, r]), initial=0.0) <= tol, (name, n, r)


def test_iris_matrix_of_the_issue_leaves_out_no_row(gpu, lowered):
    """``default_rng(0).uniform([4.3, 2.0, 1.0, 0.1], [7.9, 4.4, 6.9, 2.5], (4096, 4))`` rounded to
    fp32: no row of it has its two most probable classes closer than GAP in the oracle, so the
    label, the winner's index and its probability are compared on every row."""
    compiled, plan, _ = lowered["linear_classification"]
    X = iris_rows(4096, seed=0)
    P = np.asarray(compiled.result(X).probs, dtype=np.float64)
    srt = -np.sort(-P, axis=1)
    gap = srt[:, 0] - srt[:, 1]
    assert not ((gap > 0) & (gap < GAP)).any()
    _, _, wide = plan.score_outputs(X)
    wide = wide.cpu().numpy()
    _, _, cols = compiled.outputs_matrix_oracle(X)
    j = plan.names.index("label")
    assert np.array_equal(wide[:, j], cols["label"])
    assert np.array_equal(wide[:, len(plan.names)], P.argmax(axis=1).astype(np.float32))
    # tests/test_gpu_svm_lr.py: iris logistic probabilities, atol=2e-5
    assert np.abs(wide[:, len(plan.names) + plan.top_k] - P.max(axis=1)).max() <= 2e-5


def test_forest_vote_ties_exercise_the_tie_rule(gpu, lowered):
    """33-tree forests tie their votes often (about a tenth of the rows with 3 classes, over a third
    with 16): those rows stay in and the lower class wins on both sides."""
    from flink_jpmml_amd.bench.synth import stream_matrix

    X = stream_matrix(4096, 8, seed=2, missing_rate=0.02)
    for name, least in (("forest_votes", 0.05), ("forest_16_classes", 0.2)):
        compiled, plan, _ = lowered[name]
        res = compiled.result(X)
        P = np.asarray(res.probs)
        srt = -np.sort(-P, axis=1)
        tied = (srt[:, 0] == srt[:, 1]) & res.valid
        assert tied.mean() >= least, (name, tied.mean())
        _, _, wide = plan.score_outputs(X)
        wide = wide.cpu().numpy()
        j = plan.names.index("label")
        _, _, cols = compiled.outputs_matrix_oracle(X)
        assert np.array_equal(wide[tied, j], cols["label"][tied], equal_nan=True)
        top0 = wide[:, len(plan.names)]
        assert np.array_equal(top0[tied], P.argmax(axis=1)[tied].astype(np.float32))


# --------------------------------------------------------------------------- streaming


def _csr(X):
    from flink_jpmml_amd.api.batch import SparseRecordBatch

    keep = ~np.isnan(X)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return SparseRecordBatch(indptr, np.nonzero(keep)[1].astype(np.int32), X[keep].astype(np.float32), X.shape[1])


@pytest.fixture(scope="module")
def streaming(gpu):
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.config import ScoringConfig

    text, _, _, _, _ = FAMILIES["forest_votes"]
    cfg = ScoringConfig(device=gpu, micro_batch=4096, pipeline_depth=3, fallback="error")
    model = PmmlModel.from_string(text).bind(gpu, cfg)
    assert model.on_device
    X = _inputs("forest_votes", 10_001)
    s, v, outs = model.predict_batch_outputs(X, device=gpu, top_k=3)
    return model, X, (s.cpu().numpy(), v.cpu().numpy(), outs.numpy())


@pytest.mark.parametrize("source", ["pinned", "pageable", "device", "sparse"])
def test_predict_records_with_outputs_equals_the_synchronous_route(gpu, streaming, source):
    import torch

    from flink_jpmml_amd.api.batch import RecordBatch

    model, X, (s, v, outs) = streaming
    batch = {"pinned": lambda: RecordBatch(torch.from_numpy(X).pin_memory()),
             "pageable": lambda: RecordBatch(X),
             "device": lambda: RecordBatch(torch.from_numpy(X).to(gpu)),
             "sparse": lambda: _csr(X)}[source]()
    pb = model.predict_records(batch, outputs=True, top_k=3)
    assert np.array_equal(pb.valid, v) and np.array_equal(bits(pb.scores), bits(s))
    got = pb.outputs
    assert got.names == outs.names and got.categories == outs.categories
    assert np.array_equal(bits(got.matrix), bits(outs.matrix))
    assert np.array_equal(got.top_index, outs.top_index)
    assert np.array_equal(bits(got.top_probability), bits(outs.top_probability))
    assert got.decode("label")[:50] == outs.decode("label")[:50]
    # outputs=False on the same scorer afterwards: the plain plan
    plain = model.predict_records(batch)
    s0, v0 = model.compiled.plan(gpu).score(X)
    assert plain.outputs is None
    assert np.array_equal(plain.valid, v0.cpu().numpy()) and np.array_equal(bits(plain.scores), bits(s0.cpu().numpy()))


def test_dsl_udf_returns_outputs(gpu, tmp_path):
    from flink_jpmml_amd import ModelReader
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.bench.synth import iris_logistic_pmml
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.stream import StreamExecutionEnvironment

    path = tmp_path / "iris.pmml"
    path.write_text(iris_logistic_pmml())
    X = iris_rows(4096)
    cfg = ScoringConfig(device=gpu, micro_batch=1024, fallback="error")
    env = StreamExecutionEnvironment(config=cfg)
    out = env.from_batches(X, batch_rows=1500).evaluate(
        ModelReader(str(path)), lambda b, m: (m.on_device, m.predict_records(b, outputs=True))).collect()
    assert len(out) == 3 and all(on for on, _ in out)
    got = np.concatenate([pb.outputs.matrix for _, pb in out])
    assert not np.concatenate([pb.valid for _, pb in out]).any()  # string labels: EmptyScore, as ever
    _, _, cols = PmmlModel.from_string(iris_logistic_pmml()).compiled.outputs_matrix_oracle(X)
    want = np.stack([cols[k] for k in cols], axis=1)
    # tests/test_gpu_svm_lr.py: iris logistic probabilities, atol=2e-5
    assert got.shape == want.shape and np.abs(got - want).max() <= 2e-5


def test_replicated_plan_without_the_document_says_so(gpu):
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.api.exceptions import UnsupportedFeatureException
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.bench.synth import iris_logistic_pmml
    from flink_jpmml_amd.runtime.engine import StreamingScorer
    from flink_jpmml_amd.runtime.plans import DevicePlan

    plan = PmmlModel.from_string(iris_logistic_pmml()).compiled.plan(gpu)
    replica = DevicePlan.from_state(*plan.export_state(), gpu)  # what a rank that never parsed the document holds
    scorer = StreamingScorer(replica, micro_batch=1024)
    X = iris_rows(100)
    with pytest.raises(UnsupportedFeatureException) as e:
        scorer.submit_batch(RecordBatch(X), outputs=True)
    assert "replication" in str(e.value)
    s0, v0 = plan.score(X)
    pb = scorer.submit_batch(RecordBatch(X))
    assert np.array_equal(pb.valid, v0.cpu().numpy()) and np.array_equal(bits(pb.scores), bits(s0.cpu().numpy()))


# --------------------------------------------------------------------------- fallback


def test_fallback_policy_for_outputs_that_do_not_lower(gpu):
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.bench.synth import mixed_records, scorecard_pmml
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.runtime.plans import NotLowerable

    X = mixed_records(300, 4, seed=3, missing_rate=0.02)[1].astype(np.float32)
    strict = PmmlModel.from_string(scorecard_pmml()).bind(gpu, ScoringConfig(device=gpu, fallback="error"))
    assert strict.on_device
    with pytest.raises(NotLowerable) as e:
        strict.predict_records(RecordBatch(X), outputs=True)
    assert "RC1" in str(e.value)
    host = PmmlModel.from_string(scorecard_pmml()).bind(gpu, ScoringConfig(device=gpu, fallback="host"))
    assert host.on_device
    pb = host.predict_records(RecordBatch(X), outputs=True)
    s, v, cols = host.compiled.outputs_matrix_oracle(X)
    assert np.array_equal(pb.valid, v)
    for k in cols:
        assert np.array_equal(pb.outputs[k], cols[k], equal_nan=True)
    assert pb.outputs.decode("RC1") == [host.compiled.schema.decode("RC1", float(c)) for c in cols["RC1"]]
    plain = host.predict_records(RecordBatch(X))  # scoring itself stays on the device
    s0, v0 = host.compiled.plan(gpu).score(X)
    assert np.array_equal(bits(plain.scores), bits(s0.cpu().numpy()))
