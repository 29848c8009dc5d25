"""linear_wide.hip (dense regression tables past 16 x 128, on the matrix cores) against the float64
reference of tests/_epilogue_cases.py on exact-eta probes: every product and partial sum is an exact
fp32 number in any order, so an index, padding, slice, tail or mask error is a whole-step difference.
Comparison rules: ``test_gpu_epilogue._check``. Then one case of inexact inputs against the forward
error bound of an fp32 dot product, and a naive Bayes document end to end through the design path."""

import functools

import numpy as np
import pytest
import torch

from tests import _epilogue_cases as E
from tests import _exact as X_
from tests import test_gpu_epilogue as G

from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.bench import synth
from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.compiled import CompiledPmml

pytestmark = pytest.mark.gpu

F32 = np.float32
# (K, F, norm, sparse): the kernel's edges (column blocks per wave, slices, tails, mask words)
SHAPES = [(17, 34, "softmax", False), (33, 66, "logit", False), (33, 33, "none", True), (65, 130, "simplemax", False),
          (129, 129, "softmax", True), (256, 40, "softmax", False), (3, 129, "cauchit", False), (2, 1024, "logit", False),
          (0, 129, "none", False), (0, 1024, "none", False)]
ROW_COUNTS = (1, 63, 64, 65, 257)  # around one 64-row tile, then five tiles with a ragged last one
GUARD = float(F32(1e30))  # no probe value: etas are multiples of 1/16 up to 120, +-FLT_MAX or infinite


@functools.lru_cache(maxsize=None)
def wide_case(K, F, norm, sparse=False, zero=None):
    case = E.classification_case(K, F, norm, sparse, zero) if K else E.regression_case(F, norm)
    return case, CompiledPmml.from_string(case.probe.pmml()), case.reference(fp32_rule=True)


def _launch(plan, Xt, C):
    """Outputs of one launch; the mirrors carry the same bits and the guard rows around ``probs`` stay."""
    n = Xt.shape[0]
    s, v = plan.alloc_outputs(n)
    s2, v2 = plan.alloc_outputs(n)
    guarded = torch.full((n + 2, C), GUARD, dtype=torch.float32, device=Xt.device)
    plan.launch(Xt, s, v, probs=guarded[1:n + 1], score2=s2, valid2=v2)
    torch.cuda.synchronize()
    s, v, g = s.cpu().numpy(), v.cpu().numpy().astype(bool), guarded.cpu().numpy()
    assert np.array_equal(X_.bits(s2.cpu().numpy()), X_.bits(s)) and np.array_equal(v2.cpu().numpy().astype(bool), v)
    assert (g[0] == GUARD).all() and (g[-1] == GUARD).all() and not (g[1:-1] == GUARD).any()
    return s, v, g[1:-1]


@pytest.mark.parametrize("K,F,norm,sparse", SHAPES, ids=[f"K{k}-F{f}-{n}{'-sparse' if s else ''}" for k, f, n, s in SHAPES])
def test_exact_eta_probes(gpu, K, F, norm, sparse):
    case, c, ref = wide_case(K, F, norm, sparse)
    plan = c.plan(gpu)
    assert type(plan) is PL.LinearWidePlan and (plan.listed is not None) == sparse
    assert plan.epi_args["mode"] == E.epilogue_mode(K, norm)
    if not K:
        assert ref["flagged"].any()  # FLT_MAX + FLT_MAX: the fp32 model-value rule
    if sparse:
        assert np.isinf(case.X).any()
    C, kw = max(K, 1), dict(exact_values=True) if not K else {}
    runs = [(lay, slice(None)) for lay in (G.LAYOUTS if (K, F) in ((17, 34), (33, 66)) else G.LAYOUTS[:1])]
    runs += [("contiguous", slice(0, n)) for n in (ROW_COUNTS if (K, F) == (33, 66) else ())]
    worst = 0.0
    for layout, rows in runs:
        s, v, probs = _launch(plan, G._view(case.X[rows], layout, gpu), C)
        worst = max(worst, G._check(f"{case.name} {layout} {rows}", s, v, probs if K else None, ref, K, norm, rows, **kw))
    print(f"{case.name}: {len(case.X)} rows, largest ratio {worst:.3f} x 2^-24"
          + (f" (bound {E.C_BOUND['softmax']} measured at <= 16 classes)" if norm == "softmax" else ""))


def test_explicit_zero_coefficient_still_meets_infinity(gpu):
    """Table 0 lists field 16 (the carrier of table 16, which takes +-inf) with ``coefficient="0"``:
    0 * inf voids those rows, as in the oracle; without the entry they score."""
    case, c, ref = wide_case(33, 33, "logit", True, (16, 0))
    s, v, probs = _launch(c.plan(gpu), G._view(case.X, "contiguous", gpu), 33)
    G._check(case.name, s, v, probs, ref, 33, "logit")
    inf_rows = np.isinf(case.X[:, 16]) & ~case.miss  # a copy of one of them has a missing cell
    assert inf_rows.sum() >= 2 and not v[inf_rows].any()
    plain, c0, pref = wide_case(33, 33, "logit", True)
    _, v0, _ = _launch(c0.plan(gpu), G._view(plain.X, "contiguous", gpu), 33)
    assert np.array_equal(plain.X, case.X, equal_nan=True) and v0[inf_rows].all() and pref["valid"][inf_rows].all()


def test_inexact_inputs_within_the_dot_product_bound(gpu):
    """40 tables x 200 fields of standard normals, link ``none``: ``probs`` are the linear predictors.
    Each within (F + 2) 2^-24 (|b_k| + sum_f |W_fk| |x_f|) of the float64 product, the forward error
    bound of an fp32 dot product in any order; labels where the reference's top-two gap is clear of it."""
    K, F, n = 40, 200, 1000
    rng = np.random.default_rng(5)
    p = E.Probe(F, K, "none")
    p.W, p.b = rng.standard_normal((F, K)).astype(F32).astype(np.float64), rng.standard_normal(K).astype(F32).astype(np.float64)
    X = rng.standard_normal((n, F)).astype(F32)
    plan = CompiledPmml.from_string(p.pmml()).plan(gpu)
    assert type(plan) is PL.LinearWidePlan
    s, v, probs = _launch(plan, G._view(X, "contiguous", gpu), K)
    X64 = X.astype(np.float64)
    ref = X64 @ p.W + p.b
    bound = (F + 2) * 2.0 ** -24 * (np.abs(p.b)[None] + np.abs(X64) @ np.abs(p.W))
    err = np.abs(probs.astype(np.float64) - ref)
    print(f"largest error / bound {np.max(err / bound):.4f}")
    assert v.all() and (err <= bound).all()
    top = np.sort(ref, axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * bound.max(axis=1)
    assert clear.mean() >= 0.99
    assert np.array_equal(s[clear], (10.0 * (ref.argmax(axis=1) + 1)).astype(F32)[clear])


def test_naive_bayes_through_the_design_path(gpu):
    """A 20-class naive Bayes over 40 Gaussian inputs and a categorical one lowers to 123 design
    columns x 20 tables: validity on every row, labels and top-3 where the oracle's top-two gap exceeds 1e-3."""
    model = PmmlModel.from_string(synth.naive_bayes_pmml(n_features=40, classes=20))
    c = model.compiled
    X = synth.mixed_records(1000, 40, seed=3)[1].astype(F32)
    so, vo, po = E.oracle(c, X)
    plan = c.plan(gpu)
    assert type(plan).__name__ == "DerivedPlan" and type(plan.inner) is PL.LinearWidePlan
    Xt = torch.from_numpy(X).to(gpu)
    s, v = plan.alloc_outputs(len(X))
    probs = torch.empty((len(X), 20), dtype=torch.float32, device=gpu)
    plan.launch(Xt, s, v, probs=probs)
    s2, v2, outs = model.predict_batch_outputs(Xt, device=gpu, top_k=3)
    torch.cuda.synchronize()
    s, v, probs = s.cpu().numpy(), v.cpu().numpy().astype(bool), probs.cpu().numpy()
    assert np.array_equal(v, vo) and np.array_equal(v2.cpu().numpy().astype(bool), vo) and vo.any()
    top = np.sort(po, axis=1)
    clear = vo & (top[:, -1] - top[:, -2] > 1e-3)
    assert clear.sum() >= 0.99 * vo.sum()
    assert np.array_equal(s[clear], so[clear].astype(F32)) and np.array_equal(s2.cpu().numpy()[clear], s[clear])
    assert np.array_equal(outs.numpy().top_index[clear], np.argsort(-po, axis=1, kind="stable")[clear, :3])
    worst = np.abs(probs[vo] - po[vo]).max()
    print(f"naive Bayes 123 x 20: largest |device - oracle| probability {worst:.3e}")
    assert worst <= NB_BOUND


# 4 x the largest |device - oracle| probability measured on the MI355X (7.924e-06, docs/PARITY.md), rounded up:
# the log-likelihood sums reach several hundred in fp32 before the softmax
NB_BOUND = 3.2e-5
