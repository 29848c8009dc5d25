"""The predicate-VM tree kernel (``tree.hip``: ``gen_eval`` / ``gen_walk`` / ``gen_mixture`` /
``tree_general_kernel``) on the probes of tests/_general_cases.py, against the float64 oracle:
validity identical on all 2049 rows, scores and labels bit for bit on every valid row, class means
bit for bit for the integer-payload forest. tests/test_general_cases.py (CPU) holds the conditions
that make this a probe: what the rows reach, and that each named error changes a result."""

import numpy as np
import pytest
import torch

from tests import _general_cases as G
from tests._exact import strided

pytestmark = pytest.mark.gpu
F32 = np.float32


def _plan(cs, gpu):
    plan = cs.compiled.plan(gpu)
    inner = getattr(plan, "inner", plan)  # set splits and leaf columns add a derive pass
    assert type(inner).__name__ == "TreePlan" and inner.layout == "general", cs.name
    assert (inner.n_features > 64) == (cs.F > 64)  # F = 66: the lazy per-read feature path
    return plan, inner


def _launch(plan, gpu, X, n_probs=0, wide=False):
    Xn = np.array(X, dtype=F32)
    Xt = torch.from_numpy(strided(Xn)).to(gpu)[:, : Xn.shape[1]] if wide else torch.from_numpy(Xn).to(gpu)
    s, v = plan.alloc_outputs(len(Xn))
    p = torch.full((len(Xn), n_probs), -7.0, dtype=torch.float32, device=gpu) if n_probs else None
    plan.launch(Xt, s, v, **({"probs": p} if n_probs else {}))
    torch.cuda.synchronize()
    return s.cpu().numpy(), v.cpu().numpy().astype(bool), (p.cpu().numpy() if n_probs else None)


def _assert_same(cs, s, v, p=None):
    ref, vref, probs = cs.oracle
    assert np.array_equal(v, vref), f"{cs.name}: validity differs on {(v != vref).sum()} of {len(v)} rows"
    if p is not None:
        assert np.array_equal(p[vref], probs[vref].astype(F32)), f"{cs.name}: class means differ from the oracle"
        top = np.sort(probs[vref], axis=1)
        clear = top[:, -1] > top[:, -2]  # an exact tie has no one label
        assert clear.sum() >= vref.sum() // 2
        assert np.array_equal(s[vref][clear].astype(F32), ref[vref][clear].astype(F32)), f"{cs.name}: labels differ"
        return
    bad = np.nonzero(s[vref].astype(F32) != ref[vref].astype(F32))[0]
    assert len(bad) == 0, f"{cs.name}: {len(bad)} of {int(vref.sum())} valid rows differ from the oracle"


@pytest.mark.parametrize("key", G.ALL_CASES, ids=[G.case_id(k) for k in G.ALL_CASES])
def test_general_kernel_on_boundary_inputs(gpu, key):
    cs = G.case(*key)
    plan, inner = _plan(cs, gpu)
    if cs.family == "dist":
        assert inner.P == 3
        _assert_same(cs, *_launch(plan, gpu, cs.X, n_probs=3))
    else:
        s, v = plan.score(np.array(cs.X))
        torch.cuda.synchronize()
        _assert_same(cs, s.cpu().numpy(), v.cpu().numpy().astype(bool))


@pytest.mark.parametrize("key", G.STRIDED, ids=[G.case_id(k) for k in G.STRIDED])
def test_general_kernel_reads_strided_rows(gpu, key):
    """The rows as a view of a wider matrix: a kernel that ignores the row stride reads 97.0."""
    cs = G.case(*key)
    plan, _ = _plan(cs, gpu)
    s, v, _ = _launch(plan, gpu, cs.X, wide=True)
    _assert_same(cs, s, v)


def test_general_plan_state_round_trip(gpu):
    """What a rank that never parsed the document holds: ``export_state`` -> ``from_state`` scores
    the same bits."""
    from flink_jpmml_amd.runtime.plans import DevicePlan

    cs = G.case("weighted", 66, "defaultChild", "returnLastPrediction", False)
    plan, _ = _plan(cs, gpu)
    meta, tensors = plan.export_state()
    replica = DevicePlan.from_state(meta, {k: t.clone() for k, t in tensors.items()}, gpu)
    s0, v0, _ = _launch(plan, gpu, cs.X)
    s1, v1, _ = _launch(replica, gpu, cs.X)
    _assert_same(cs, s1, v1)
    assert np.array_equal(v0, v1) and np.array_equal(s0.view(np.uint32)[v0], s1.view(np.uint32)[v1])


@pytest.mark.parametrize("key", G.MIXTURES, ids=[f"{m}-{n}-seed{s}" for s, n, m in G.MIXTURES])
def test_mixture_kernel_on_boundary_inputs(gpu, key):
    """``gen_mixture``: cells on the documents' constants +-2 ulps, a quarter missing (forks at the
    root, at depth and inside an open mixture: asserted on the CPU). Validity exact, class
    probabilities within the project's 2e-5, labels equal wherever the oracle's two best classes
    are further apart than twice that."""
    c, X, ref, vref, probs = G.mixture_case(*key)
    plan = c.plan(gpu)
    inner = getattr(plan, "inner", plan)
    assert inner.layout == "general" and inner.mix_mass is not None
    s, v, p = _launch(plan, gpu, X, n_probs=inner.C)
    assert np.array_equal(v, vref), f"validity differs on {(v != vref).sum()} rows"
    np.testing.assert_allclose(p[vref], probs[vref], rtol=0, atol=G.MIX_ATOL)
    clear = G.mixture_clear(probs, vref)
    assert 2 * int(clear.sum()) >= int(vref.sum())
    assert np.array_equal(s[clear].astype(F32), ref[clear].astype(F32))
