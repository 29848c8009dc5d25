"""Ranked entity outputs without a GPU: the row-at-a-time reference against the float64 oracle, the
numpy twin of ``ops/csrc/entities.hip`` against the reference through
``compiled.output_plan("cpu", entity_ranks=True)`` in both arithmetic forms, the twin's mutants, the
lowering limits, the default refusals and the rank-1 host columns against the parent's recording."""

import os

import numpy as np
import pytest

import _entity_cases as EC
from _entity_cases import CASES, MFMA_CASES
from flink_jpmml_amd.api.exceptions import UnsupportedFeatureException
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.bench import synth
from flink_jpmml_amd.runtime.plans import NotLowerable, lowering_dry_run

FORMS = [(n, "valu") for n in CASES] + [(n, "mfma") for n in MFMA_CASES]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "entity_rank1_parent.npz")


def _plan(compiled, variant="valu", **kw):
    with lowering_dry_run():
        return compiled.output_plan("cpu", entity_ranks=True, cluster_variant=variant, knn_variant=variant, **kw)


def _columns(plan, X):
    _, _, mat = plan.score_outputs(X)
    mat = mat.numpy() if hasattr(mat, "numpy") else np.asarray(mat)
    return {n: mat[:, i] for i, n in enumerate(plan.names)}


@pytest.fixture(scope="module")
def lowered():
    """name -> (case, compiled, probe rows, reference columns)."""
    out = {}
    for name, case in CASES.items():
        compiled = PmmlModel.from_string(EC.document(case)).compiled
        X = EC.probe_rows(case)
        out[name] = (case, compiled, X, EC.reference(case, X, compiled.schema.lookup))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_the_oracle(lowered, name):
    """``outputs_matrix_oracle`` on the batch, and ``predict_with_outputs`` row by row."""
    case, compiled, X, want = lowered[name]
    _, _, cols = compiled.outputs_matrix_oracle(X)
    EC.assert_columns(case, {k: np.asarray(v, dtype=np.float32) for k, v in cols.items()}, want, X, name)
    # the probes hold what they promise: ties, a missing field, an all-missing row, a rejected row
    assert np.isnan(X).all(axis=1).any()
    assert case["F"] == 1 or (np.isnan(X).any(axis=1) & ~np.isnan(X).all(axis=1)).any()
    ev = compiled.evaluator
    for r in (0, 3, len(X) - 1):
        P, ok = compiled.prepare(X[r: r + 1])
        res, outs = compiled.evaluate_prepared(P)
        for k, v in outs.items():
            one = np.where(ok, np.asarray(v, dtype=np.float64), np.nan)[0]
            assert (one == cols[k][r]) or (np.isnan(one) and np.isnan(cols[k][r])), (name, k, r)
    assert ev is not None


def test_probes_hold_ties_across_tiles_and_half_waves():
    case = CASES["c65x5"]
    C, _ = EC.entities(case)
    dup = {(i, j) for i in range(len(C)) for j in range(i + 1, len(C)) if (C[i] == C[j]).all()}
    assert any(j - i == 4 for i, j in dup) and any(j - i == 32 for i, j in dup)
    three = [i for i in range(len(C)) if sum((C[i] == C[j]).all() for j in range(len(C))) >= 3]
    assert three, "no three-way tie among the centres"


@pytest.mark.parametrize("name,variant", FORMS)
def test_twin_equals_the_reference(lowered, name, variant):
    case, compiled, X, want = lowered[name]
    plan = _plan(compiled, variant)
    assert plan.entities is not None and plan.entities.variant == variant
    assert plan.entities.knn == (case["kind"] == "knn" and case["k"] > 1)
    EC.assert_columns(case, _columns(plan, X), want, X, (name, variant))


def test_dry_run_equals_the_host_path(lowered):
    """The public host route (``device=None``) and the dry-run plan give the same decoded ids."""
    case, compiled, X, _ = lowered["k5n33_ids"]
    model = PmmlModel.from_string(EC.document(case))
    _, _, outs = model.predict_batch_outputs(X)
    got = _columns(_plan(compiled), X)
    ids = outs.decode("o1")
    assert ids[0] is not None and ids[0].startswith("i") and ids[16] is None  # strings; None on a NaN row
    from flink_jpmml_amd.api.batch import BatchOutputs

    plan = _plan(compiled)
    mat = np.stack([got[n] for n in plan.names], axis=1)
    back = BatchOutputs(plan.names, mat.astype(np.float64), compiled.schema, None, None, None)
    assert back.decode("o1") == ids and back.decode("o5") == outs.decode("o5")


def test_one_nn_answers_instance_ids_not_targets(lowered):
    case, compiled, X, _ = lowered["k1n9"]
    model = PmmlModel.from_string(EC.document(case))
    _, _, outs = model.predict_batch_outputs(X)
    ids = set(EC.instance_ids(case))
    assert {x for x in outs.decode("o0") if x is not None} <= ids
    assert not ids & {str(t) for t in EC.targets(case)}
    assert np.isnan(outs.matrix[:, outs.names.index("o2")]).all()  # rank 2 of a 1-NN: past the list


def test_instance_id_variable_is_parsed():
    with_ids = PmmlModel.from_string(EC.document(CASES["k5n33_ids"])).compiled.model
    without = PmmlModel.from_string(EC.document(CASES["k8n65_rows"])).compiled.model
    assert with_ids.instance_id_variable == "rowid" and with_ids.instance_ids[:2] == ["i0", "i1"]
    assert without.instance_id_variable is None and without.instance_ids[:3] == ["1", "2", "3"]


# --------------------------------------------------------------------------- mutants


def _shows(monkeypatch, lowered, changes, E, names) -> bool:
    for attr, fn in changes.items():
        monkeypatch.setattr(E, attr, fn)
    for name, variant in names:
        case, compiled, X, want = lowered[name]
        try:
            EC.assert_columns(case, _columns(_plan(compiled, variant), X), want, X, name)
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize("mutant", ["ties to the higher index", "unfinished affinity", "rank off by one",
                                    "named column swapped", "half-wave merge dropped"])
def test_every_mutant_shows(monkeypatch, lowered, mutant):
    muts, E = EC.mutants()
    where = {"named column swapped": [("c9x5_named", "valu"), ("c9x5_named", "mfma")],
             "half-wave merge dropped": [("c33x5_interval", "mfma"), ("k8n65_rows", "mfma")],
             "unfinished affinity": [("c2x5", "valu"), ("k8n65_rows", "valu")]}
    names = where.get(mutant, [("c33x5_interval", "valu"), ("k5n33_ids", "valu"), ("c65x5", "mfma")])
    assert _shows(monkeypatch, lowered, muts[mutant], E, names), mutant


def test_target_used_as_id_shows(monkeypatch, lowered):
    from flink_jpmml_amd.runtime import entities as RE

    monkeypatch.setattr(RE, "entity_ids", lambda ev: list(ev.entity_ids))  # a k-NN's entity_ids are its targets
    case, _, X, _ = lowered["k1n9"]
    compiled = PmmlModel.from_string(EC.document(case)).compiled  # not the cached plan
    want = EC.reference(case, X, compiled.schema.lookup)
    with pytest.raises(AssertionError):
        EC.assert_columns(case, _columns(_plan(compiled), X), want, X, "k1n9")


# --------------------------------------------------------------------------- limits and refusals


def _refused(text: str, **kw) -> str:
    compiled = PmmlModel.from_string(text).compiled
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        compiled.output_plan("cpu", **kw)
    return str(e.value)


def _with(case: dict, **kw) -> str:
    return EC.document(dict(case, **kw))


def test_limits_name_the_field():
    c = CASES["c65x5"]
    msg = _refused(_with(c, out=[("entityId", 33, None, "string")]), entity_ranks=True)
    assert "'o0'" in msg and "rank 33 > 32" in msg
    many = [("affinity", 2 + (i % 30), None, "double") for i in range(65)]
    msg = _refused(_with(c, out=many), entity_ranks=True)
    assert "'o64'" in msg and "more than 64 entity columns" in msg
    big = dict(CASES["k5n33_ids"], out=[("entityId", 1, None, "integer")])
    text = EC.document(big).replace("<rid>100</rid>", "<rid>16777217</rid>")
    msg = _refused(text, entity_ranks=True)
    assert "'o0'" in msg and "fp32 cannot hold exactly" in msg
    named = dict(CASES["k5n33_ids"], out=[("affinity", 1, "i3", "double")])
    msg = _refused(EC.document(named), entity_ranks=True)
    assert "'o0'" in msg and "named training instance" in msg
    with pytest.raises(UnsupportedFeatureException):  # the host keeps no [n, N] matrix either
        PmmlModel.from_string(EC.document(named)).compiled.outputs_matrix_oracle(EC.probe_rows(named))


def test_class_outputs_of_a_knn_classifier_stay_refused():
    text = synth.knn_pmml(n_instances=40, k=3).replace(
        "</MiningSchema>", '</MiningSchema>\n  <Output><OutputField name="near" feature="entityId" rank="1" '
        'dataType="string" optype="categorical"/><OutputField name="lab" feature="predictedValue" '
        'dataType="string" optype="categorical"/></Output>', 1)
    msg = _refused(text, entity_ranks=True)
    assert "'lab'" in msg and "has no index mode" in msg


def test_switch_off_refuses_as_before():
    knn = synth.knn_pmml(n_instances=40, k=3).replace(
        "</MiningSchema>", '</MiningSchema>\n  <Output><OutputField name="near" feature="entityId" '
        'dataType="string" optype="categorical"/></Output>', 1)
    assert _refused(knn) == "output 'near': KnnPlan has no index mode (class / entity outputs are host-only)"
    assert _refused(EC.document(CASES["k5n33_ids"])) == \
        "output 'o1': entityId (entity ranks) of this model is host-only"
    assert _refused(EC.document(CASES["c33x5_interval"])) == "output 'o2': rank 2 > 1 is not evaluated"
    only_named = dict(CASES["c9x5_named"], out=[("entityId", 1, None, "string")])
    assert _refused(EC.document(only_named)) == "output 'n0': affinity of the named entity '1' is host-only"


def test_switch_is_part_of_the_cache_key_and_the_config():
    from flink_jpmml_amd.config import ScoringConfig

    compiled = PmmlModel.from_string(EC.document(dict(CASES["c9x5_named"], name_all=False,
                                                      out=[("entityId", 1, None, "string")]))).compiled
    with lowering_dry_run():
        a = compiled.output_plan("cpu")
        b = compiled.output_plan("cpu", entity_ranks=True)
        assert a is not b and b.entities is None  # rank 1, unnamed: stays a column of outputs_kernel
        assert compiled.output_plan("cpu", entity_ranks=True) is b
    assert ScoringConfig().entity_ranks is False and ScoringConfig(entity_ranks=True).entity_ranks is True
    old = os.environ.get("FJA_ENTITY_RANKS")
    try:
        os.environ["FJA_ENTITY_RANKS"] = "1"
        assert ScoringConfig.from_env().entity_ranks is True
        os.environ["FJA_ENTITY_RANKS"] = "0"
        assert ScoringConfig.from_env().entity_ranks is False
    finally:
        if old is None:
            os.environ.pop("FJA_ENTITY_RANKS", None)
        else:
            os.environ["FJA_ENTITY_RANKS"] = old


def test_other_models_ignore_the_switch():
    compiled = PmmlModel.from_string(synth.iris_logistic_pmml()).compiled
    with lowering_dry_run():
        assert compiled.output_plan("cpu", entity_ranks=True).entities is None


# --------------------------------------------------------------------------- the host against the parent


def test_rank_one_host_columns_are_the_parents(lowered):
    """Rank-1 columns of the clustering documents, bit for bit what the commit before this feature
    computed (``tests/golden/entity_rank1_parent.npz``, float64)."""
    rec = np.load(GOLDEN)
    seen = 0
    for name, (case, _, X, _) in lowered.items():
        if case["kind"] != "cluster":
            continue
        # a fresh schema: a string field's codes follow the order of its first lookups
        compiled = PmmlModel.from_string(EC.document(case)).compiled
        _, _, cols = compiled.outputs_matrix_oracle(X)
        for oname, _, rank, value, _ in EC.outputs(case):
            if rank == 1 and value is None:
                want = rec[f"{name}|{oname}"]
                assert np.array_equal(np.asarray(cols[oname], dtype=np.float64).view(np.uint64),
                                      want.view(np.uint64)), (name, oname)
                seen += 1
    assert seen == len(rec.files) and seen >= 10


# --------------------------------------------------------------------------- inexact inputs: the condition


@pytest.mark.parametrize("name", sorted(EC.INEXACT))
def test_inexact_inputs_keep_within_their_cap(name):
    """At most 1 % of the rows may drop out of the index comparison per rank, from the oracle alone."""
    spec = EC.INEXACT[name]
    compiled = PmmlModel.from_string(spec["text"]).compiled
    X = EC.inexact_rows(spec)
    dropped = EC.undecided(compiled, X, spec["ranks"])
    assert dropped.shape == (len(spec["ranks"]), len(X))
    assert dropped.mean(axis=1).max() <= 0.01, (name, dropped.mean(axis=1))
