"""Scorecard reason codes without a GPU: the row-at-a-time reference against the float64 oracle, the
numpy twin of ``ops/csrc/reasons.hip`` against the reference through
``compiled.output_plan("cpu", reason_codes=True)``, the twin's mutants, the lowering limits and the
default refusal."""

import numpy as np
import pytest

import _reason_cases as RC
from _reason_cases import CASES, MUTANTS, bits

NAMES = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def lowered():
    """name -> (case, compiled, dry-run output plan, reference codes, reference valid)."""
    out = {}
    for c in CASES:
        compiled, plan = RC.dry_plan(RC.document(c))
        codes, valid = RC.reference(c, compiled)
        out[c["name"]] = (c, compiled, plan, codes, valid)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_oracle(lowered, name):
    case, compiled, _, codes, valid = lowered[name]
    P, ok = compiled.prepare(case["X"])
    res, _ = compiled.evaluate_prepared(P)
    assert np.array_equal(valid, np.asarray(res.valid, dtype=bool) & ok)
    rc = res.extra.get("reason_codes")
    if not compiled.model.use_reason_codes:
        assert rc is None
        return
    assert valid.any()
    for r in np.flatnonzero(valid):
        assert codes[r] == rc[r], (name, r, case["X"][r])


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_the_reference_through_the_output_plan(lowered, name):
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    case, compiled, plan, codes, valid = lowered[name]
    want = RC.expected_matrix(case, compiled, codes, valid)
    with lowering_dry_run():
        _, v, matrix = plan.score_outputs(case["X"])
    assert plan.names == [f"RC{r}" for r in case["kw"]["ranks"]]
    assert np.array_equal(np.asarray(v), valid)
    got = np.asarray(matrix)
    for j, nm in enumerate(plan.names):
        assert np.array_equal(bits(got[:, j]), bits(want[:, j])), (name, nm)
    if compiled.model.use_reason_codes:
        assert plan.reasons is not None and case["what"].startswith("shared" if plan.reasons.shared else "disjoint")
        assert not np.isnan(want).all()
    else:
        assert plan.reasons is None and np.isnan(got).all()


def test_cases_place_what_they_claim(lowered):
    """The situations the case table names do occur in the reference's rankings."""
    def ranks(name):
        case, _, _, codes, valid = lowered[name]
        return {tuple(case["X"][r]): codes[r] for r in np.flatnonzero(valid)}

    assert ranks("equal_diffs")[(0, 0, 0)] == ["C", "B", "A"]  # three equal differences: characteristic order
    assert ranks("equal_diffs")[(3, 2, 1)] == ["A", "B", "C"]  # 5 > 0 > -2
    assert ranks("shared_tie")[(0, 0, 0)] == ["S", "T"] and ranks("shared_tie")[(0, 1, 0)] == ["T", "S"]
    assert ranks("flip_touch")[(0, 0, 0)] == ["Z", "A", "Q"] and ranks("flip_touch")[(1, 1, 0)] == ["A", "Z", "Q"]
    assert ranks("signed_zero")[(0, 0, 0)] == ["A", "B", "C"]
    assert ranks("fp32_rounding")[(0, 0)] == ["B", "A"]
    assert ranks("order3")[(0, 0, 0, 0)] == ["T", "S"] and ranks("order3")[(0, 1, 1, 0)] == ["T", "S"]
    assert ranks("no_codes")[(1, 0, 0)] == ["C"] and ranks("no_codes")[(0, 1, 1)] == ["X", "C"]
    assert ranks("char_baseline")[(0, 0, 0)][0] == "B"
    assert ranks("prep")[(0, 0, 1)] == ["A", "B", "M"] and ranks("prep")[(1, 1, 3)] == ["B", "A", "S"]


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_shows(lowered, mutant):
    """A twin with one rule changed differs from the twin in a compared value on some case."""
    shown = []
    for name, (case, compiled, plan, _, _) in lowered.items():
        if plan.reasons is None:
            continue
        good = RC.twin(plan, case["X"])
        bad = MUTANTS[mutant](case, plan)
        if not np.array_equal(bits(good), bits(bad)):
            shown.append(name)
    assert shown, mutant


def test_the_twin_does_not_depend_on_its_tile(lowered):
    for name in ("prep", "codes64_shared", "complex"):
        case, _, plan, _, _ = lowered[name]
        base = RC.twin(plan, case["X"])
        for rows in (64, 128, 256):
            if name == "codes64_shared" and rows != 64:
                continue
            assert np.array_equal(bits(RC.twin(plan, case["X"], rows=rows)), bits(base))


def test_geometry_keeps_one_workgroup_inside_64_kib():
    from flink_jpmml_amd.ops import reasons as R

    assert R.geometry(8, 64, False) == (256, True)
    assert R.geometry(9, 64, True) == (64, True)  # 64 codes x 12 bytes x 64 rows = 48 KiB + the planes
    assert R.geometry(64, 8, False) == (256, True) and R.geometry(65, 8, False) == (128, True)
    assert R.geometry(300, 8, False) == (256, False)  # the planes never fit: features from global memory
    assert R.geometry(300, 64, True) == (64, False)
    for F, C, shared in ((8, 64, False), (9, 64, True), (65, 8, False), (300, 64, True)):
        rows, lds = R.geometry(F, C, shared)
        assert R.lds_bytes(F, C, rows, shared, lds) <= R.LDS_BYTES
    assert [R.template_k(k) for k in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    with pytest.raises(ValueError):
        R.template_k(9)


def test_tables_refuse_indices_outside_their_tables(lowered):
    T = lowered["prep"][2].reasons
    for over in (dict(n_code=T.n_code - 1), dict(n_feat=T.n_feat - 1), dict(width=1),
                 dict(preds=T.preds[:-1]), dict(tables=T.tables[:-1]), dict(dval=T.dval[:-1]),
                 dict(n_code=65)):
        with pytest.raises(ValueError):
            RC.retabled(T, **over)


# --------------------------------------------------------------------------- limits and the switch


def _refused(text, field, **kw):
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.runtime.plans import NotLowerable, lowering_dry_run

    compiled = PmmlModel.from_string(text).compiled
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        compiled.output_plan("cpu", **kw)
    assert repr(field) in str(e.value), str(e.value)
    return str(e.value)


def test_limits_raise_not_lowerable_naming_the_field():
    assert "rank" in _refused(RC.with_ranks("codes64", (1, 9)), "RC9", reason_codes=True)
    assert "65 distinct reason codes" in _refused(RC.too_many_codes(), "RC1", reason_codes=True)
    assert "baselineScore" in _refused(RC.no_baseline(), "RC1", reason_codes=True)


def test_lds_limit_raises_not_lowerable_naming_the_field(monkeypatch):
    from flink_jpmml_amd.ops import reasons as R

    monkeypatch.setattr(R, "LDS_BYTES", 64 * 64 * 12 - 1)  # 64 rows of 64 accumulators no longer fit
    assert "LDS" in _refused(RC.document(RC.CASE["codes64_shared"]), "RC1", reason_codes=True)
    RC.dry_plan(RC.document(RC.CASE["codes64"]))  # the register path asks for no accumulators


def test_rank_8_lowers_and_65_codes_do_not(lowered):
    assert lowered["codes64"][2].reasons.k == 8 and lowered["codes64"][2].reasons.n_code == 64
    assert lowered["codes64_shared"][2].reasons.n_code == 64 and lowered["codes64_shared"][2].reasons.shared


def test_the_default_call_still_refuses():
    _refused(RC.document(RC.CASE["equal_diffs"]), "RC1")
    _refused(RC.document(RC.CASE["equal_diffs"]), "RC1", reason_codes=False)
    assert "rank" in _refused(RC.with_ranks("equal_diffs", (2,)), "RC2")


def test_reason_codes_on_another_model_changes_nothing():
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.bench.synth import iris_logistic_pmml
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    compiled = PmmlModel.from_string(iris_logistic_pmml()).compiled
    with lowering_dry_run():
        a = compiled.output_plan("cpu")
        b = compiled.output_plan("cpu", reason_codes=True)
    assert a is not b and b.reasons is None  # reason_codes is part of the cache key
    assert np.array_equal(a.prog_np, b.prog_np) and a.names == b.names and a.kernel_dst == b.kernel_dst
    with lowering_dry_run():
        assert compiled.output_plan("cpu", reason_codes=True) is b


def test_every_code_is_registered_at_lowering():
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    compiled = PmmlModel.from_string(RC.document(RC.CASE["flip_touch"])).compiled
    with lowering_dry_run():
        compiled.output_plan("cpu", reason_codes=True)
    for name in ("RC1", "RC2"):
        assert compiled.schema.values[name] == ["Z", "A", "Q"]  # document order, before the first batch


def test_config_switch():
    from flink_jpmml_amd.config import ScoringConfig

    assert ScoringConfig().reason_codes is False and ScoringConfig(reason_codes=True).reason_codes is True
    import os
    old = os.environ.get("FJA_REASON_CODES")
    try:
        os.environ["FJA_REASON_CODES"] = "1"
        assert ScoringConfig.from_env().reason_codes is True
        os.environ["FJA_REASON_CODES"] = "0"
        assert ScoringConfig.from_env().reason_codes is False
    finally:
        if old is None:
            os.environ.pop("FJA_REASON_CODES", None)
        else:
            os.environ["FJA_REASON_CODES"] = old


def test_synth_scorecard_equals_the_host_path_on_mixed_rows():
    """``synth.scorecard_pmml()`` (interval bins, a compound ``and``, set and equality attributes on a
    string field, attribute-level codes, a characteristic baseline): 600 rows with missing values."""
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.bench.synth import mixed_records, scorecard_pmml
    from flink_jpmml_amd.runtime.outputs import host_batch_outputs
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    compiled = PmmlModel.from_string(scorecard_pmml()).compiled
    X = mixed_records(600, 4, seed=11, missing_rate=0.05)[1].astype(np.float32)
    with lowering_dry_run():
        plan = compiled.output_plan("cpu", reason_codes=True)
        _, v, matrix = plan.score_outputs(X)
    _, hv, outs = host_batch_outputs(compiled, X)
    assert np.array_equal(np.asarray(v), hv) and 0 < hv.sum() < len(X)
    got = np.asarray(matrix).astype(np.float64)
    assert outs.names == plan.names == ["RC1", "RC2"]
    assert np.array_equal(got, outs.matrix, equal_nan=True)
    assert len({x for x in outs.decode("RC1") if x is not None}) >= 4
