"""rbf.hip (radial-basis-function networks on the matrix cores) against the float64 oracle at the
shapes where the kernel can break: one unit, a ragged last hidden tile, every input bucket, the
full 32-unit output tile and the limits; 1, 63, 65 and 257 rows with a missing input, a row on a
centre and (simplemax) a row every unit underflows on. Then the public routes."""

import functools

import numpy as np
import pytest
import torch

from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.bench import synth
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.nn_plans import RbfPlan, _affine_of

pytestmark = pytest.mark.gpu

# (n_in, H, n_out, hidden norm, classification, altitude)
CASES = [(1, 1, 1, None, False, 1.0), (3, 33, 1, "simplemax", False, 1.0), (17, 32, 1, "softmax", False, 1.0),
         (24, 70, 5, "simplemax", True, 1.0), (40, 96, 3, None, True, 1.0), (17, 64, 32, None, True, 1.0),
         (128, 1024, 1, "softmax", False, 1.0), (3, 5, 2, None, True, 1.05)]
ROWS = (1, 63, 65, 257)
NAN_ROW, CENTRE_ROW, FAR_ROW = 70, 100, 200


@functools.lru_cache(maxsize=None)
def case(n_in, H, n_out, norm, cls, alt):
    """The compiled document, 257 rows with the planted ones, and the oracle's result on them."""
    c = CompiledPmml.from_string(synth.rbf_pmml(n_in, H, n_out, seed=n_in + H, classification=cls,
                                                normalization=norm, altitude=alt))
    X = synth.stream_matrix(257, n_in, seed=H)
    X[NAN_ROW, n_in // 2] = np.nan
    maps = [_affine_of(inp.derived.expression) for inp in c.evaluator.nn.inputs]
    centre = c.evaluator.rbf_layers()["centers"][H // 2]
    X[CENTRE_ROW] = [(w - sh) / sc for w, (sc, sh, _) in zip(centre, maps)]
    if norm == "simplemax":
        X[FAR_ROW] = 1e4  # every activation underflows in float64 as well: 0 / 0
    s, v = c.score_matrix_oracle(X)
    return c, X, s, v, c.result(X).probs


@pytest.mark.parametrize("n_in,H,n_out,norm,cls,alt", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}" for c in CASES])
def test_kernel_against_the_oracle(gpu, n_in, H, n_out, norm, cls, alt):
    c, X, want, valid, P = case(n_in, H, n_out, norm, cls, alt)
    plan = c.plan(gpu)
    assert type(plan) is RbfPlan
    assert not valid[NAN_ROW] and valid[CENTRE_ROW] and (norm != "simplemax" or cls or not valid[FAR_ROW])
    for n in ROWS:
        Xt = torch.from_numpy(X[:n]).to(gpu)
        s, v = plan.alloc_outputs(n)
        probs = torch.full((n, n_out), 7.0, dtype=torch.float32, device=gpu) if cls else None
        plan.launch(Xt, s, v, probs=probs)
        torch.cuda.synchronize()
        s, v = s.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(bool)
        assert np.array_equal(v, valid[:n]), f"{n} rows: validity at {np.flatnonzero(v != valid[:n])}"
        assert np.isnan(s[~v]).all()
        if not cls:
            err, scale = np.abs(s[v] - want[:n][v]).max(initial=0.0), max(1.0, np.abs(want[:n][v]).max(initial=0.0))
            print(f"{n} rows: |gpu - oracle| {err:.3g}, scale {scale:.3g}")
            assert err < 1e-4 * scale
            continue
        got, ref = probs.cpu().numpy().astype(np.float64), P[:n]
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        fin = ~np.isnan(ref)
        err, scale = np.abs(got[fin] - ref[fin]).max(initial=0.0), max(1.0, np.abs(ref[fin]).max(initial=0.0))
        top = np.sort(np.where(fin, ref, -np.inf), axis=1)
        clear = v & ((top[:, -1] - top[:, -2]) > 2e-4)
        print(f"{n} rows: |gpu - oracle| {err:.3g} on the probabilities, {np.mean(~clear[v]):.3%} rows left out")
        assert err < 1e-4 * scale
        assert np.array_equal(s[clear], want[:n][clear]) and (~clear[v]).mean() <= 0.02


def test_treated_inputs_take_the_prepare_pass(gpu):
    """A MiningField with ``missingValueReplacement``: ``_with_prepared_inputs`` puts the derive pass
    in front, the RBF kernel reads prepared columns and the replaced row scores."""
    doc = synth.rbf_pmml(6, 40, 1, seed=5, normalization="simplemax")
    c = CompiledPmml.from_string(doc.replace('<MiningField name="f2"/>',
                                             '<MiningField name="f2" missingValueReplacement="0.25"/>'))
    X = synth.stream_matrix(65, 6, seed=9)
    X[3, 2] = X[9, 4] = np.nan
    want, valid = c.score_matrix_oracle(X)
    plan = c.plan(gpu)
    assert type(plan).__name__ == "DerivedPlan" and type(plan.inner) is RbfPlan
    s, v = plan.score(X)
    s, v = s.cpu().numpy().astype(np.float64), v.cpu().numpy()
    assert valid[3] and not valid[9] and np.array_equal(v, valid)
    assert np.abs(s[v] - want[v]).max() < 1e-4 * max(1.0, np.abs(want[v]).max())


def test_predict_batch_on_the_device(gpu):
    c, X, want, valid, _ = case(3, 33, 1, "simplemax", False, 1.0)
    model = PmmlModel.from_string(synth.rbf_pmml(3, 33, 1, seed=36, normalization="simplemax"))
    s, v = model.predict_batch(X, device=gpu)
    s, v = s.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(bool)
    assert np.array_equal(v, valid) and np.abs(s[v] - want[v]).max() < 1e-4 * max(1.0, np.abs(want[v]).max())


def test_class_outputs_and_top_k_against_the_host_route(gpu):
    _, X, _, valid, _ = case(24, 70, 5, "simplemax", True, 1.0)
    X = X[valid & (np.arange(257) != FAR_ROW)]
    model = PmmlModel.from_string(synth.rbf_pmml(24, 70, 5, seed=94, classification=True, normalization="simplemax"))
    hs, hv, host = model.predict_batch_outputs(X, top_k=2)
    ds, dv, dev = model.predict_batch_outputs(X, device=gpu, top_k=2)
    assert np.array_equal(dv.cpu().numpy().astype(bool), hv) and hv.all()
    tp, hp = dev.top_probability.cpu().numpy().astype(np.float64), np.asarray(host.top_probability)
    assert np.abs(tp - hp).max() < 1e-4
    clear = (hp[:, 0] - hp[:, 1]) > 2e-4
    assert np.array_equal(dev.top_index.cpu().numpy()[clear], np.asarray(host.top_index)[clear])
    assert np.array_equal(ds.cpu().numpy()[clear], hs[clear].astype(np.float32)) and (~clear).mean() <= 0.02


def test_a_refused_network_falls_back_to_the_host(gpu):
    """A third layer: ``RbfPlan`` refuses with ``NotLowerable``, so ``fallback="host"`` applies."""
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.runtime import engine
    from flink_jpmml_amd.utils.metrics import METRICS
    from tests.test_rbf import REFUSED

    c = CompiledPmml.from_string(REFUSED["more than two layers"])
    before = METRICS.counters.get("scoring.host_fallback_models", 0)
    sc = engine.make_scorer(c, gpu, ScoringConfig(device=gpu, fallback="host"))
    assert sc.kind == "host" and METRICS.counters["scoring.host_fallback_models"] == before + 1
