"""Association rules on the device path, on the host: the independent reference of
``_rule_cases.py`` = the float64 oracle = the numpy twin of ``rules.hip`` = the ``OutputPlan`` dry run,
on every row of every column of every case, bit for bit; the tallies of what the cases place; the
mutants; the limits; the switch."""

import numpy as np
import pytest

import _rule_cases as RC
from flink_jpmml_amd.api.batch import BatchOutputs
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.runtime.plans import NotLowerable, lowering_dry_run

NAMES = [c["name"] for c in RC.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_reference_oracle_twin_and_dry_run_agree(name):
    case = RC.CASE[name]
    cols, _ = RC.expected(name)
    model, plan = RC.dry_plan(name)
    schema = model.compiled.schema
    X = case["X"]
    # the float64 host oracle
    s, v, host = model.predict_batch_outputs(X)
    assert np.isnan(s).all() and not v.any()
    assert RC.compare(case, cols, np.asarray(host.matrix), host.decode) == [], name
    # the numpy twin of the kernel, straight over the packed tables
    t = RC.twin(plan, X)
    assert RC.compare(case, cols, t, BatchOutputs(plan.names, t, schema).decode) == [], name
    # the plan's dry run
    with lowering_dry_run():
        ds, dv, wide = plan.score_outputs(X)
    wide = np.asarray(wide)
    assert np.isnan(np.asarray(ds)).all() and not np.asarray(dv).any()
    assert np.array_equal(RC.bits(wide), RC.bits(t))
    assert RC.compare(case, cols, wide, BatchOutputs.from_wide(plan.names, wide, 0, schema).decode) == [], name
    # string columns hold the same encodings on both paths
    assert np.array_equal(RC.bits(np.asarray(host.matrix)), RC.bits(wide))


def test_every_placed_situation_is_tallied():
    seen = set()
    for name in NAMES:
        seen |= RC.expected(name)[1]
    missing = [f for f in RC.REQUIRED if f not in seen]
    assert missing == []
    # the tie rule is only visible when document order is not sorted order
    plan = RC.dry_plan("i64")[1]
    assert any(list(o) != sorted(o) for o in plan.rules.order)


def test_geometry_covers_the_three_workgroup_sizes_and_both_basket_homes():
    from flink_jpmml_amd.ops import rules as K

    geo = {name: (K.geometry(p.rules.n_feat, p.rules.n_items), K.words(p.rules.n_items) <= K.REG_WORDS)
           for name, p in ((n, RC.dry_plan(n)[1]) for n in NAMES)}
    assert geo["f128"] == (64, True) and geo["f64"] == (128, False)
    assert geo["i128"] == (256, True) and geo["i129"] == (256, False) and geo["i1024"] == (256, False)
    assert {K.template_r(RC.dry_plan(n)[1].rules.k) for n in NAMES} == {1, 2, 4, 8}


@pytest.mark.parametrize("mutant", list(RC.MUTANTS))
def test_mutants_change_a_compared_value(mutant):
    name, run = RC.MUTANTS[mutant]
    case = RC.CASE[name]
    _, plan = RC.dry_plan(name)
    good = RC.twin(plan, case["X"])
    assert not np.array_equal(RC.bits(run(case, plan)), RC.bits(good)), mutant
    assert np.array_equal(RC.bits(RC.twin(plan, case["X"])), RC.bits(good))  # and leaves nothing behind


def _refused(text, field):
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        PmmlModel.from_string(text).compiled.output_plan("cpu", association_rules=True)
    assert repr(field) in str(e.value), str(e.value)
    return str(e.value)


def _small(name="lim", n_items=4, n_rules=3, slots=2, outputs=None, **kw):
    return RC.make_case(name, n_items, n_rules, slots, outputs or [RC.out("first"), RC.out("second", "ruleId")], 5,
                        n_rows=6, **kw)


def test_limits_name_the_field():
    from flink_jpmml_amd.ops import rules as K

    assert (K.MAX_ITEMS, K.MAX_RULES, K.MAX_SET_ITEMS, K.MAX_FIELDS, K.MAX_RANK, K.MAX_GROUPS, K.MAX_COLUMNS) == \
        (1024, 4096, 16, 128, 8, 4, 64)
    assert "1025 items" in _refused(RC.document(_small(n_items=1025)), "first")
    assert "4097 rules" in _refused(RC.document(_small(n_rules=4097)), "first")
    assert "17 items" in _refused(RC.document(_small(n_items=33, set_sizes=(17,), pool=20)), "first")
    assert "129 active fields" in _refused(RC.document(_small(slots=129)), "first")
    assert "rank 9" in _refused(RC.document(_small(outputs=[RC.out("first"), RC.out("ninth", rank=9)])), "ninth")
    many = [RC.out(f"c{j}", rank=1 + j % 8) for j in range(65)]
    assert "64 rule columns" in _refused(RC.document(_small(outputs=many)), "c64")
    text, field = RC.five_groups()
    assert "more than 4 distinct" in _refused(text, field)
    assert "no rules" in _refused(RC.document(_small(n_rules=0)), "first")
    odd = [RC.out("first"), RC.out("odd", algorithm="best")]
    assert "algorithm 'best'" in _refused(RC.document(_small(outputs=odd)), "odd")
    assert "ruleFeature 'colour'" in _refused(RC.document(_small(outputs=[RC.out("odd", "colour")])), "odd")
    assert "top_k" in str(pytest.raises(NotLowerable, _top_k).value)


def _top_k():
    with lowering_dry_run():
        PmmlModel.from_string(RC.document(_small())).compiled.output_plan("cpu", top_k=2, association_rules=True)


def test_an_encoding_fp32_cannot_hold_is_refused(monkeypatch):
    compiled = PmmlModel.from_string(RC.document(_small())).compiled
    real = compiled.schema.lookup
    monkeypatch.setattr(compiled.schema, "lookup",
                        lambda n, v: float(2 ** 24 + 1) if n == "second" else real(n, v))
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        compiled.output_plan("cpu", association_rules=True)
    assert "'second'" in str(e.value) and "fp32" in str(e.value)


def test_four_groups_lower_and_launch_arguments_are_checked():
    from flink_jpmml_amd.ops import rules as K

    T = RC.dry_plan("i33")[1].rules
    assert len(T.groups) == 4
    with pytest.raises(ValueError):  # a pair outside the basket never reaches a launch
        pairs = T.pairs.copy()
        pairs[0, 0] = K.words(T.n_items)
        RC.retabled(T, pairs=pairs)
    with pytest.raises(ValueError):
        cols = T.cols.copy()
        cols[0, 3] = T.width
        RC.retabled(T, cols=cols)
    with pytest.raises(ValueError):
        RC.retabled(T, order=T.order[:, :-1])


def test_switch_off_is_the_parent_behaviour():
    compiled = RC.model("i31").compiled
    with lowering_dry_run(), pytest.raises(NotLowerable) as e:
        compiled.output_plan("cpu")
    assert str(e.value) == "model has no target field (every record scores EmptyScore)"
    # and the host path of a bound model is untouched
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.config import ScoringConfig

    case = RC.CASE["i31"]
    m = PmmlModel.from_string(RC.document(case)).bind(None, ScoringConfig(association_rules=True))
    assert m.scorer.kind == "null" and m.scorer.rule_plan is None
    pb = m.predict_records(RecordBatch(case["X"]), outputs=True)
    cols, _ = RC.expected("i31")
    assert RC.compare(case, cols, np.asarray(pb.outputs.matrix), pb.outputs.decode) == []


def test_switch_is_ignored_by_other_models():
    from flink_jpmml_amd.bench.synth import kmeans_pmml

    compiled = PmmlModel.from_string(kmeans_pmml(5, 4, seed=3)).compiled
    X = np.random.default_rng(0).normal(size=(33, 4)).astype(np.float32)
    with lowering_dry_run():
        a = compiled.output_plan("cpu", association_rules=True)
        b = compiled.output_plan("cpu")
        assert a is not b and a.rules is None and type(a.inner) is type(b.inner)
        ra = [np.asarray(t) for t in a.score_outputs(X)]
        rb = [np.asarray(t) for t in b.score_outputs(X)]
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y, equal_nan=True)


def test_config_reads_the_environment(monkeypatch):
    from flink_jpmml_amd.config import ScoringConfig

    assert ScoringConfig().association_rules is False
    monkeypatch.delenv("FJA_ASSOCIATION_RULES", raising=False)
    assert ScoringConfig.from_env().association_rules is False
    monkeypatch.setenv("FJA_ASSOCIATION_RULES", "1")
    assert ScoringConfig.from_env().association_rules is True
    monkeypatch.setenv("FJA_ASSOCIATION_RULES", "off")
    assert ScoringConfig.from_env().association_rules is False
