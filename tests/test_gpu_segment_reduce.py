"""``ops/csrc/segment.hip`` (``segment_reduce_kernel<64, 64>`` / ``<256, 256>``) and its tensor-op
fallback against the float64 oracle, bit for bit (GPU half of ``tests/test_segment_cases.py``).

A / B: the real plan of every case of ``tests/_segment_cases.py`` with the device stand-ins swapped
in for its segment plans, launched once on the whole matrix — through the fused reduction kernel
(A) and, with ``_red`` switched off, through the tensor ops that deep predicates fall back to (B).
C: ``nullPrediction`` documents through the real tree kernels, all segments in one
``tree_pointer_multi_kernel`` launch and one launch per segment. Every comparison is validity with
``np.array_equal`` and scores on their fp32 bit patterns, NaN where the oracle has no score; no row
is left out."""

import functools

import numpy as np
import pytest
import torch

from flink_jpmml_amd.config import ScoringConfig
from flink_jpmml_amd.runtime.plans import TreePlan
from tests import _segment_cases as SC

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in SC.all_cases()]


def _plan(txt, gpu, **opts):
    """The real plan, lowered once per document (``CompiledPmml.plan`` caches it)."""
    return SC.compiled(txt).plan(gpu, **ScoringConfig(device=gpu, fallback="error").lowering_opts(), **opts)


@pytest.mark.parametrize("path", ["kernel", "tensor-ops"])
@pytest.mark.parametrize("name", NAMES)
def test_reduction_on_prescribed_segment_results(gpu, name, path):
    case = SC.case(name)
    plan = _plan(case.txt, gpu)
    seg = SC.segmented(plan)
    assert seg._red is not None and seg._red["stride"] == (65 if case.K <= 64 else 257)
    ref, vref = SC.reference(case)
    red = seg._red
    try:
        if path == "tensor-ops":
            seg._red = None
        for strided in (False, True):
            s, v, s2, v2 = SC.run_plan(plan, case, gpu, strided=strided, mirrors=True)
            what = f"{name} {path}{' strided' if strided else ''}"
            SC.assert_same(s, v, ref, vref, what)
            assert np.array_equal(SC.bits(s2), SC.bits(s)) and np.array_equal(v2, v), f"{what}: mirrors"
    finally:
        seg._red = red


# --------------------------------------------------------------------------- real segment kernels


@functools.lru_cache(maxsize=None)
def _real_reference(method, classification, treatment):
    txt = SC.real_doc(method, classification, treatment)
    X = SC.real_inputs(txt)
    ref, vref = SC.compiled(txt).score_matrix_oracle(X)
    return txt, X, ref, vref


def _launch(plan, X, gpu):
    Xt = torch.from_numpy(np.array(X)).to(gpu)
    s = torch.full((len(X),), -7.0, dtype=torch.float32, device=gpu)
    v = torch.full((len(X),), 9, dtype=torch.uint8, device=gpu)
    plan.launch(Xt, s, v)
    torch.cuda.synchronize()
    return s.cpu().numpy(), v.cpu().numpy().astype(bool)


@pytest.mark.parametrize("method,classification", SC.REAL)
def test_segments_that_yield_nothing_through_the_tree_kernels(gpu, method, classification):
    """Segment trees with ``missingValueStrategy="nullPrediction"`` on inputs at their cuts: applying
    segments write ``V = 0``, once from one multi-segment launch and once from a launch each."""
    vrefs = {}
    for treatment in SC.TREATMENTS:
        txt, X, ref, vref = _real_reference(method, classification, treatment)
        assert 0 < vref.mean() < 1
        vrefs[treatment] = vref
        plan = _plan(txt, gpu)
        seg = SC.segmented(plan)
        assert seg._red is not None and all(isinstance(p, TreePlan) for p in seg.subs)
        s, v = _launch(plan, X, gpu)
        assert sum(len(g["idx"]) for g in seg._multi) == seg.n_subs  # every tree segment, one launch
        SC.assert_same(s, v, ref, vref, f"{method} {treatment} multi")
        each = _plan(txt, gpu, layout="perfect")
        seg = SC.segmented(each)
        assert seg._red is not None and all(isinstance(p, TreePlan) and p.layout == "perfect" for p in seg.subs)
        s, v = _launch(each, X, gpu)
        assert seg._multi == []  # no pointer-layout member: a launch per segment
        SC.assert_same(s, v, ref, vref, f"{method} {treatment} per segment")
    if method != "selectFirst":  # selectFirst takes the first applying segment under every treatment
        assert (vrefs[None] != vrefs["skipSegment"]).any()
