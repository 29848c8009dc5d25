"""Lowering of dense regression tables past linear.hip's 16 tables x 128 fields: ``compile_plan``
routes them to ``LinearWidePlan`` (csrc/linear_wide.hip, 256 x 1024), smaller shapes stay on
``LinearPlan``, larger ones stay refused. CPU only, under ``lowering_dry_run()``."""

import numpy as np
import pytest
import torch

from tests import _epilogue_cases as E

from flink_jpmml_amd.bench import synth
from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import lowering_dry_run

CPU = torch.device("cpu")
# document -> (tables, design columns) of the wide plan it must reach
WIDE = {
    "naive-bayes-40x20": (lambda: synth.naive_bayes_pmml(n_features=40, classes=20), 20, 123),
    "multinomial-6x24": (lambda: synth.glm_pmml("multinomialLogistic", n_features=6, classes=24), 24, 9),
    "multinomial-150x3": (lambda: synth.glm_pmml("multinomialLogistic", n_features=150, classes=3), 3, 153),
    "design-softmax-8x20": (lambda: synth.regression_design_pmml(n_features=8, classes=20, normalization="softmax"),
                            20, 11),
    "dense-129x2-logit": (lambda: E.Probe(129, 2, "logit").pmml(), 2, 129),
    "dense-34x17-softmax": (lambda: E.Probe(34, 17, "softmax").pmml(), 17, 34),
}


def _plan(text: str):
    with lowering_dry_run():
        plan = PL.compile_plan(CompiledPmml.from_string(text), CPU)
    return getattr(plan, "inner", plan)


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_tables_reach_the_wide_plan(name):
    doc, K, F = WIDE[name]
    plan = _plan(doc())
    assert type(plan) is PL.LinearWidePlan and plan.kind == "linear_wide"
    assert (plan.K, plan.n_features) == (K, F)
    assert plan.W.shape == (plan.Fp, plan.Kp) == (-(-F // 32) * 32, -(-K // 32) * 32)
    assert not plan.W[F:].any() and not plan.W[:, K:].any() and not plan.b[K:].any()


def test_limits_on_both_sides():
    assert type(_plan(E.Probe(128, 16, "softmax").pmml())) is PL.LinearPlan  # still linear.hip
    assert type(_plan(E.Probe(1024, 2, "logit").pmml())) is PL.LinearWidePlan
    for F, K in ((34, 257), (1025, 2)):
        with pytest.raises(PL.NotLowerable):
            _plan(E.Probe(F, K, "softmax").pmml())


def test_listed_words_name_the_builders_predictors():
    """33 sparse tables: bit k % 32 of word k // 32 of row f is the builder's ``listed[f, k]`` (the
    33rd table needs the second word); a dense document carries no mask."""
    p = E.Probe(66, 33, "none", sparse=True, zero_coef=(1, 0))
    plan = _plan(p.pmml())
    words = plan.listed.numpy().view(np.uint32)
    assert words.shape == (66, 2)
    bits = (words[:, np.arange(64) // 32] >> (np.arange(64) % 32).astype(np.uint32)) & 1
    assert np.array_equal(bits[:, :33].astype(bool), p.listed) and not bits[:, 33:].any()
    assert _plan(E.Probe(34, 17, "softmax").pmml()).listed is None


def test_state_round_trip(monkeypatch):
    from flink_jpmml_amd.ops import _lib

    monkeypatch.setattr(_lib, "load", lambda: None)  # from_state binds the library: not needed to compare tensors
    plan = _plan(E.Probe(66, 33, "softmax", sparse=True).pmml())
    meta, tensors = plan.export_state()
    twin = PL.DevicePlan.from_state(meta, tensors, CPU)
    assert type(twin) is PL.LinearWidePlan
    for k in PL.LinearWidePlan._STATE:
        a, b = getattr(plan, k), getattr(twin, k)
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, k
