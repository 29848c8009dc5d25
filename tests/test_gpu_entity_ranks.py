"""Ranked entity outputs on the MI355X: ``pmml_entities_launch`` through ``OutputPlan.launch`` and
``predict_batch_outputs`` against the row-at-a-time reference on the exact documents (bit for bit;
4 fp32 ulps on the affinities of rows with a missing field), against the plan's own winner on random
inputs (no tolerance), and against the float64 oracle on inexact inputs."""

import numpy as np
import pytest

import _entity_cases as EC
from _entity_cases import CASES, INEXACT, MFMA_CASES, TOL
from _exact import bits, strided
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.bench import synth

pytestmark = pytest.mark.gpu

GUARD = 7.0
ROW_COUNTS = (1, 63, 64, 65, 257)
FORMS = [(n, "valu") for n in CASES] + [(n, "mfma") for n in MFMA_CASES]


@pytest.fixture(scope="module")
def lowered():
    """name -> (case, compiled, probe rows, reference columns): computed once, never changed."""
    out = {}
    for name, case in CASES.items():
        compiled = PmmlModel.from_string(EC.document(case)).compiled
        X = EC.probe_rows(case)
        want = EC.reference(case, X, compiled.schema.lookup)
        for v in want.values():
            v.setflags(write=False)
        out[name] = (case, compiled, X, want)
    return out


def _plan(compiled, gpu, variant):
    return compiled.output_plan(gpu, entity_ranks=True, cluster_variant=variant, knn_variant=variant)


def _cycled(want, n, m):
    idx = np.arange(n) % m
    return {k: v[idx] for k, v in want.items()}


def _columns(plan, mat):
    mat = mat.cpu().numpy()
    return {n: mat[:, i] for i, n in enumerate(plan.names)}


@pytest.mark.parametrize("name,variant", FORMS)
def test_exact_documents(gpu, lowered, name, variant):
    import torch

    case, compiled, X, want = lowered[name]
    plan = _plan(compiled, gpu, variant)
    assert plan.entities is not None and plan.entities.variant == variant
    for n in ROW_COUNTS:
        Xn = EC.take_rows(X, n)
        _, _, mat = plan.score_outputs(Xn)
        torch.cuda.synchronize()
        EC.assert_columns(case, _columns(plan, mat), _cycled(want, n, len(X)), Xn, (name, variant, n))


@pytest.mark.parametrize("name,variant", [("c9x5_named", "valu"), ("c33x5_interval", "mfma"), ("k5n33_ids", "valu"),
                                          ("k8n65_rows", "mfma"), ("k1n9", "valu")])
def test_public_route(gpu, lowered, name, variant):
    case, _, X, _ = lowered[name]
    model = PmmlModel.from_string(EC.document(case))  # its own schema: the id codes follow the lookups
    ref = EC.reference(case, X, model.compiled.schema.lookup)
    s, v, outs = model.predict_batch_outputs(X, device=gpu, entity_ranks=True, cluster_variant=variant,
                                             knn_variant=variant)
    got = {n: np.asarray(outs[n].cpu().numpy()) for n in outs.names}
    EC.assert_columns(case, got, ref, X, (name, variant))
    _, _, host = model.predict_batch_outputs(X)
    first_id = next(o[0] for o in EC.outputs(case) if o[1] == "entityId" and o[2] == 1)
    assert outs.decode(first_id) == host.decode(first_id)  # the id strings, None on a NaN row
    assert None in outs.decode(first_id) and any(x is not None for x in outs.decode(first_id))


@pytest.mark.parametrize("name", ["c9x5_named", "k5n33_ids"])
def test_config_switch_serves_predict_records(gpu, lowered, name):
    """``ScoringConfig(entity_ranks=True)`` with ``fallback="error"``: the record route lowers the
    document and decodes what the host decodes."""
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.config import ScoringConfig

    case, _, X, _ = lowered[name]
    model = PmmlModel.from_string(EC.document(case)).bind(
        gpu, ScoringConfig(device=gpu, entity_ranks=True, fallback="error"))
    assert model.on_device
    _, hv, host = model.predict_batch_outputs(X)
    pb = model.predict_records(RecordBatch(X), outputs=True)
    assert np.array_equal(np.asarray(pb.valid, dtype=bool), hv)
    for oname, feat, _, _, _ in EC.outputs(case):
        if feat == "entityId":
            assert pb.outputs.decode(oname) == host.decode(oname), (name, oname)
    strict = PmmlModel.from_string(EC.document(case)).bind(gpu, ScoringConfig(device=gpu, fallback="error"))
    with pytest.raises(Exception) as e:  # off: refused by name, and "error" does not fall back
        strict.predict_records(RecordBatch(X), outputs=True)
    assert "host-only" in str(e.value) or "not evaluated" in str(e.value)


@pytest.mark.parametrize("name,variant", [("c33x5_interval", "valu"), ("c65x5", "mfma"), ("k32n65x64", "mfma"),
                                          ("k5n33_ids", "valu")])
def test_layouts_guards_and_a_side_stream(gpu, lowered, name, variant):
    """A contiguous input and a column view of a wider matrix; ``outputs`` a view with guard columns
    and guard elements around it; the launch on a side stream."""
    import torch

    case, compiled, X, want = lowered[name]
    plan = _plan(compiled, gpu, variant)
    n, W, pad = 129, plan.width, 3
    Xn = EC.take_rows(X, n)
    ref = _cycled(want, n, len(X))
    side = torch.cuda.Stream(device=gpu)
    for layout in ("contiguous", "view"):
        Xt = torch.from_numpy(Xn).to(gpu) if layout == "contiguous" else \
            torch.from_numpy(strided(Xn)).to(gpu)[:, : Xn.shape[1]]
        buf = torch.full((2 + n * (W + pad) + 2,), GUARD, dtype=torch.float32, device=gpu)
        out = buf[2: 2 + n * (W + pad)].view(n, W + pad)[:, :W]
        score, valid = plan.alloc_outputs(n)
        torch.cuda.synchronize()
        plan.launch(Xt, score, valid, stream=side, outputs=out)
        side.synchronize()
        host = buf.cpu().numpy()
        body = host[2: 2 + n * (W + pad)].reshape(n, W + pad)
        assert (host[:2] == GUARD).all() and (host[-2:] == GUARD).all() and (body[:, W:] == GUARD).all(), layout
        EC.assert_columns(case, {k: body[:, i] for i, k in enumerate(plan.names)}, ref, Xn, (name, variant, layout))


def test_kernel_writes_only_its_columns(gpu, lowered):
    """``entities_launch`` alone: the matrix's other columns keep what they held."""
    import torch

    from flink_jpmml_amd.ops.entities import EntityTables, entities_launch, entities_numpy

    case, compiled, X, _ = lowered["c9x5_named"]
    T = _plan(compiled, gpu, "valu").entities
    cols = T.cols.copy()
    cols[:, 3] = 2 * np.arange(len(cols)) + 1  # every other column
    W = 2 * len(cols) + 1
    T2 = EntityTables(T.ent, T.weights, T.scales, T.qweights, T.cfun, T.metric, T.similarity, T.p, cols, T.named,
                      T.tables, T.k, T.knn, W)
    out = torch.full((len(X), W), GUARD, dtype=torch.float32, device=gpu)
    entities_launch(torch.from_numpy(X).to(gpu), out, T2)
    torch.cuda.synchronize()
    want = entities_numpy(X, np.full((len(X), W), GUARD, dtype=np.float32), T2)
    got = out.cpu().numpy()
    assert (got[:, 0::2] == GUARD).all()
    assert np.array_equal(bits(got), bits(want))


# --------------------------------------------------------------------------- consistency with the plan

METRICS = ("squaredEuclidean", "euclidean", "cityBlock", "chebychev", 'minkowski p-parameter="3"')
COMPARES = ("absDiff", "gaussSim", "delta", "equal")


def _rows(F, n=300, seed=13):
    X = synth.stream_matrix(n, F, seed=seed, missing_rate=0.05)
    X[7] = np.nan
    X[11] = X[12]  # a repeated row
    return X


@pytest.mark.parametrize("metric", METRICS)
def test_rank_one_is_the_cluster_plans_winner(gpu, metric):
    """Every compare function, distance and similarity, both variants: rank-1 index == the plan's
    ``label`` and rank-1 affinity bits == the plan's ``affinity`` on every row."""
    import torch

    from flink_jpmml_amd.ops.entities import ENT_AFFINITY, ENT_ID, EntityTables, entities_launch

    K_, F = 33, 6
    X = _rows(F)
    Xt = torch.from_numpy(X).to(gpu)
    for compare in COMPARES:
        for kind in ("distance", "similarity"):
            text = synth.kmeans_pmml(K_, F, seed=3, metric=metric, weighted=True, compare=compare) \
                .replace('kind="distance"', f'kind="{kind}"')
            mfma = kind == "distance" and compare == "absDiff" and metric in METRICS[:2]
            for variant in ("valu", "mfma") if mfma else ("valu",):
                compiled = PmmlModel.from_string(EC.with_ranked_outputs(text, (1, 2), ("3",))).compiled
                base = compiled.plan(gpu, cluster_variant=variant)
                s, v = base.alloc_outputs(len(X))
                label = torch.full((len(X),), -7, dtype=torch.int32, device=gpu)
                aff = torch.full((len(X),), GUARD, dtype=torch.float32, device=gpu)
                base.launch(Xt, s, v, label=label, affinity=aff)
                plan = _plan(compiled, gpu, variant)
                T = plan.entities
                assert T.variant == variant == base.variant and not T.knn
                _, _, mat = plan.score_outputs(X)
                # rank 1 from the entity kernel itself (the plan leaves rank 1 to outputs_kernel):
                # the plan's tables with the columns {index of rank 1, affinity of rank 1}
                T1 = EntityTables(T.ent, T.weights, T.scales, T.qweights, T.cfun, T.metric, T.similarity, T.p,
                                  [(ENT_ID, 0, 0, 0), (ENT_AFFINITY, 0, 0, 1)], np.full(K_, -1),
                                  np.arange(K_, dtype=np.float32), T.k, False, 2, wc=T.wc, cc=T.cc)
                own = torch.full((len(X), 2), GUARD, dtype=torch.float32, device=gpu)
                entities_launch(Xt, own, T1, prep=plan.inner.prep)
                torch.cuda.synchronize()
                got = _columns(plan, mat)
                own = own.cpu().numpy()
                ok = v.cpu().numpy() != 0
                what = (metric, compare, kind, variant)
                assert ok.sum() >= len(X) - 2 and not ok[7], what
                assert np.isnan(own[~ok]).all(), what
                assert np.array_equal(own[ok, 0], label.cpu().numpy()[ok].astype(np.float32)), what
                assert np.array_equal(bits(own[ok, 1]), bits(aff.cpu().numpy()[ok])), what
                assert np.isnan(got["id1"][~ok]).all() and np.isnan(got["aff1"][~ok]).all(), what
                assert np.array_equal(got["id1"][ok] - 1.0, label.cpu().numpy()[ok].astype(np.float32)), what
                assert np.array_equal(bits(got["aff1"][ok]), bits(aff.cpu().numpy()[ok])), what
                # rank 1 of this kernel and the rank-1 column of outputs_kernel are the same row by row
                third = got["named3"]
                is3 = ok & (got["id1"] == 3.0)
                assert np.array_equal(bits(third[is3]), bits(got["aff1"][is3])), what


@pytest.mark.parametrize("metric", METRICS)
def test_neighbours_reproduce_the_knn_plans_score(gpu, metric):
    """``KnnPlan`` exposes no label: its average over the k targets, summed in rank order in fp32,
    is reproduced in every bit from the neighbours this kernel names — same neighbours, same order."""
    import torch

    N, F, k = 70, 5, 5
    X = _rows(F)
    for compare in COMPARES:
        for kind in ("distance", "similarity"):
            text = synth.knn_pmml(N, F, k=k, classification=False, seed=4, metric=metric, measure=kind,
                                  compare=compare)
            mfma = kind == "distance" and compare == "absDiff" and metric in METRICS[:2]
            for variant in ("valu", "mfma") if mfma else ("valu",):
                compiled = PmmlModel.from_string(EC.with_ranked_outputs(text, range(1, k + 1))).compiled
                base = compiled.plan(gpu, knn_variant=variant)
                s, v = base.score(X)
                plan = _plan(compiled, gpu, variant)
                assert plan.entities.knn and plan.entities.variant == variant == base.variant
                _, _, mat = plan.score_outputs(X)
                torch.cuda.synchronize()
                got = _columns(plan, mat)
                ok = v.cpu().numpy() != 0
                what = (metric, compare, kind, variant)
                assert ok.sum() >= len(X) - 2 and not ok[7], what
                y = compiled.evaluator.inst_value.astype(np.float32)
                acc = np.zeros(int(ok.sum()), dtype=np.float32)
                for r in range(1, k + 1):
                    assert np.isnan(got[f"id{r}"][~ok]).all() and not np.isnan(got[f"id{r}"][ok]).any(), what
                    acc = (acc + y[got[f"id{r}"][ok].astype(np.int64) - 1]).astype(np.float32)
                assert np.array_equal(bits(acc / np.float32(k)), bits(s.cpu().numpy()[ok])), what
                a = np.stack([got[f"aff{r}"][ok] for r in range(1, k + 1)], axis=1)
                d = np.diff(a, axis=1)
                assert ((d <= 0) if kind == "similarity" else (d >= 0)).all(), what


# --------------------------------------------------------------------------- inexact inputs against the oracle


@pytest.mark.parametrize("name", sorted(INEXACT))
def test_inexact_inputs_against_the_oracle(gpu, name):
    """Affinities of every rank within rtol = atol = 2e-5 of the oracle's distance to the entity the
    device named; the entity itself compared where the oracle decides the rank (at most 1 % of the
    rows drop out per rank). Named affinities alike."""
    import torch

    spec = INEXACT[name]
    compiled = PmmlModel.from_string(spec["text"]).compiled
    X = EC.inexact_rows(spec)
    D, key = EC.oracle_measure(compiled, X)
    order = np.argsort(key, axis=1, kind="stable")
    _, _, cols = compiled.outputs_matrix_oracle(X)
    dropped = EC.undecided(compiled, X, spec["ranks"])
    assert dropped.mean(axis=1).max() <= 0.01
    tol = EC.inexact_tolerance(spec)
    for variant in ("valu", "mfma") if spec.get("mfma") else ("valu",):
        plan = _plan(compiled, gpu, variant)
        assert plan.entities.variant == variant
        _, _, mat = plan.score_outputs(X)
        torch.cuda.synchronize()
        got = _columns(plan, mat)
        rows = np.arange(len(X))
        for j, r in enumerate(spec["ranks"]):
            want_id = cols[f"id{r}"]
            valid = ~np.isnan(want_id)
            gid = got[f"id{r}"]
            assert np.array_equal(np.isnan(gid), ~valid), (name, variant, r)
            e = np.where(valid, gid, 1).astype(np.int64) - 1
            ref = D[rows, e]
            err = np.abs(got[f"aff{r}"].astype(np.float64) - ref)[valid]
            bound = (tol + tol * np.abs(ref))[valid]
            print(f"{name} {variant} rank {r}: worst |err| / (atol + rtol |d|) at {TOL:g} = "
                  f"{(err / (TOL + TOL * np.abs(ref[valid]))).max():.3f}, dropped {dropped[j].mean():.4f}")
            assert (err <= bound).all(), (name, variant, r, float((err / bound).max()))
            sure = valid & ~dropped[j]
            assert np.array_equal(e[sure], order[sure, r - 1]), (name, variant, r)
        for n in plan.names:
            if n.startswith("named"):
                err = np.abs(got[n].astype(np.float64) - cols[n])
                okk = ~np.isnan(cols[n])
                assert np.array_equal(np.isnan(got[n]), ~okk), (name, variant, n)
                assert (err[okk] <= tol + tol * np.abs(cols[n][okk])).all(), (name, variant, n)
