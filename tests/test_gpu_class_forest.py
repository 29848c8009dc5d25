"""The class-tile tree kernel (``ops/csrc/tree_classes.hip``) against the float64 oracle by the
exact-probe rule: dyadic vote weights and leaf probabilities of k / 64 keep every accumulator exact,
so labels and validity are equal on every row and a probability is within ``4 x 2^-24`` (one rounding
of ``1 / sum(w)``, one of the product). Shapes sit on the class quarters, tree chunks and row tiles."""

import functools
import re

import numpy as np
import pytest
import torch

from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.bench.synth import gbdt_pmml, random_forest_pmml, stream_matrix
from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.class_forest import ClassForestPlan
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from tests import _boundary as B
from tests import _epilogue_cases as E
from tests.test_class_forest import single_tree

pytestmark = pytest.mark.gpu

F = 24
PROB_BOUND = 4 * 2.0 ** -24
VOTES = ("majorityVote", "weightedMajorityVote")  # PAIR leaves; every other form has DENSE leaves


def rows(n: int, seed: int) -> np.ndarray:  # 3 % missing cells, a half-missing row, a last row missing every field
    X = stream_matrix(n, F, seed=seed, missing_rate=0.03)
    if n > 2:
        X[n // 2, 1::2] = np.nan
        X[-1, :] = np.nan
    return X


@functools.lru_cache(maxsize=None)
def forest(form: str, C: int, trees: int, depth: int, strategy: str = "defaultChild"):
    txt = random_forest_pmml(n_trees=trees, depth=depth, n_features=F, n_classes=C, seed=C + trees,
                             missing_strategy=strategy, method="average" if form == "tree" else form,
                             distributions=form not in VOTES)
    return single_tree(txt) if form == "tree" else txt


def launch(plan, X, C):
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(plan.device)
    s, v = plan.alloc_outputs(len(X))
    probs = torch.full((len(X), C), -7.0, dtype=torch.float32, device=plan.device)
    plan.launch(Xt, s, v, probs=probs)
    return s.cpu().numpy(), v.cpu().numpy().astype(bool), probs.cpu().numpy()


CASES = [  # form, classes, trees, rows, depth, missing value strategy
    ("majorityVote", 17, 1, 1, 1, "defaultChild"),
    ("majorityVote", 64, 31, 63, 6, "defaultChild"),
    ("weightedMajorityVote", 65, 33, 65, 6, "nullPrediction"),
    ("majorityVote", 256, 70, 257, 6, "nullPrediction"),
    ("average", 17, 33, 257, 6, "defaultChild"),
    ("weightedAverage", 65, 31, 63, 6, "nullPrediction"),
    ("average", 256, 70, 65, 1, "defaultChild"),
    ("tree", 64, 1, 257, 6, "defaultChild"),
    ("tree", 256, 1, 65, 6, "nullPrediction"),
]


@pytest.mark.parametrize("form,C,trees,n,depth,strategy", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_forests_equal_the_oracle(gpu, form, C, trees, n, depth, strategy):
    c = CompiledPmml.from_string(forest(form, C, trees, depth, strategy))
    X = rows(n, seed=C + n)
    so, vo, po = E.oracle(c, X)
    plan = c.plan(gpu)
    assert type(plan) is ClassForestPlan and plan.dense == (0 if form in VOTES else 1)
    assert plan.n_stage <= F and (trees * depth > 1 or plan.n_stage == 1)  # only the columns the trees read
    s, v, probs = launch(plan, X, C)
    # the all-missing row: routed by defaultChild, no prediction under nullPrediction
    assert n <= 2 or vo[-1] == (strategy == "defaultChild")
    assert np.array_equal(v, vo), f"validity differs on rows {np.flatnonzero(v != vo)[:8]}"
    assert np.array_equal(s[vo], so[vo].astype(np.float32)), f"labels differ on rows {np.flatnonzero(s != so)[:8]}"
    err = np.abs(probs[vo].astype(np.float64) - po[vo]).max() if vo.any() else 0.0
    assert err <= PROB_BOUND, f"largest probability error {err * 2 ** 24:.3f} x 2^-24"


def test_twenty_class_chain(gpu):
    """20 ensembles of 4 integer-leaf trees, intercepts k / 32: probabilities within the K-class chain
    bound of ``tests/test_gpu_epilogue.py``, labels where the oracle's two largest are twice that apart."""
    txt = B.integer_leaves(gbdt_pmml(n_trees=4, depth=4, n_features=F, objective="multiclass", n_classes=20, seed=5),
                           modulus=5)
    k = iter(range(20))
    c = CompiledPmml.from_string(re.sub(r'intercept="[^"]+"', lambda m: f'intercept="{next(k) / 32}"', txt))
    X = rows(257, seed=8)
    so, vo, po = E.oracle(c, X)
    plan = c.plan(gpu)
    assert type(plan) is ClassForestPlan and plan.dense == 0 and plan.acc_init is not None and plan.n_trees == 80
    s, v, probs = launch(plan, X, 20)
    assert np.array_equal(v, vo) and vo.all()
    bound = E.C_BOUND["softmax"] * 2.0 ** -24
    assert np.abs(probs.astype(np.float64) - po).max() <= bound
    top = np.sort(po, axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * bound
    print(f"rows left out of the label comparison: {(~clear).mean():.4f}")
    assert (~clear).mean() <= 0.02 and np.array_equal(s[clear], so[clear].astype(np.float32))


@pytest.mark.parametrize("form", ["weightedMajorityVote", "weightedAverage"])
def test_six_classes_equal_tree_plan_bit_for_bit(gpu, form):
    c = CompiledPmml.from_string(forest(form, 6, 33, 6, "nullPrediction"))
    X = rows(257, seed=6)
    (s, v, p), (s2, v2, p2) = launch(ClassForestPlan(c, gpu), X, 6), launch(PL.TreePlan(c, gpu), X, 6)
    assert 0 < v.sum() < len(v) and np.array_equal(v, v2) and np.array_equal(s, s2, equal_nan=True)
    assert np.array_equal(p[v], p2[v])  # (a row without a prediction has no probabilities)


def test_public_routes(gpu):
    """The device routes against the host route; 257 classes are refused: ``fallback="host"`` applies."""
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.runtime import engine
    from flink_jpmml_amd.utils.metrics import METRICS

    model = PmmlModel.from_string(forest("weightedAverage", 65, 31, 6))
    X = rows(65, seed=3)
    hs, hv, host = model.predict_batch_outputs(X, top_k=3)
    s, v = model.predict_batch(X, device=gpu)
    assert hv.all() and np.array_equal(v.cpu().numpy().astype(bool), hv) and np.array_equal(s.cpu().numpy(), hs)
    ds, dv, dev = model.predict_batch_outputs(X, device=gpu, top_k=3)
    assert np.array_equal(dv.cpu().numpy().astype(bool), hv) and np.array_equal(ds.cpu().numpy(), hs)
    assert np.abs(dev.top_probability.cpu().numpy() - np.asarray(host.top_probability)).max() <= PROB_BOUND
    po = np.sort(E.oracle(model.compiled, X)[2], axis=1)[:, ::-1]
    clear = (po[:, :3] - po[:, 1:4] > 2 * PROB_BOUND).all(axis=1)  # no tie among the four largest
    assert clear.any() and np.array_equal(dev.top_index.cpu().numpy()[clear], np.asarray(host.top_index)[clear])
    big = CompiledPmml.from_string(random_forest_pmml(n_trees=2, depth=2, n_features=4, n_classes=257, seed=1))
    before = METRICS.counters.get("scoring.host_fallback_models", 0)
    sc = engine.make_scorer(big, gpu, ScoringConfig(device=gpu, fallback="host"))
    assert sc.kind == "host" and METRICS.counters["scoring.host_fallback_models"] == before + 1
