"""The wide PERFECT tree kernel (csrc/tree_common.h ``wide_tile``) against the float64 oracle, bit
for bit, on the named cases of tests/_wide_cases.py (CPU twin: tests/test_wide_cases.py): every
accumulation mode, 256- / 128- / 64-row tiles, one and many chunks on both blobs, the 8 / 4 / 2 / 1
tail batches of the static and the dynamic path, split partials, both staging loops, class codes
and VOTE8 counters at and past 255 trees a group, every depth but 5 (tests/test_gpu_boundary.py).

Validity, scores and labels with ``np.array_equal`` on every row of 1, ROWS - 1, ROWS, ROWS + 1 and
2 ROWS + 33 rows and of the matrix that forces both tile paths into one launch; the one tolerance is
the softmax bound of docs/PARITY.md (9.12 x 2^-24) on the class probabilities of the K-class chains."""

import numpy as np
import pytest
import torch

from tests import _epilogue_cases as E
from tests import _exact
from tests import _wide_cases as W

from flink_jpmml_amd.runtime.plans import TreePlan

pytestmark = pytest.mark.gpu
F32 = np.float32


def _launch(plan, Xt, launch, probs=False):
    s, v = plan.alloc_outputs(Xt.shape[0])
    p = torch.full((Xt.shape[0], plan.C), -7.0, dtype=torch.float32, device=plan.device) if probs else None
    plan.launch(Xt, s, v, probs=p, **launch)
    torch.cuda.synchronize()
    return s.cpu().numpy(), v.cpu().numpy().astype(bool), None if p is None else p.cpu().numpy()


def _same(what, s, v, ref, vref):
    assert np.array_equal(v, vref), f"{what}: validity differs on rows {np.flatnonzero(v != vref)[:8]}"
    want = ref[vref].astype(F32)
    bad = np.flatnonzero(s[vref].view(np.uint32) != want.view(np.uint32))
    assert np.array_equal(s[vref].view(np.uint32), want.view(np.uint32)), \
        f"{what}: {len(bad)} of {len(want)} valid rows differ, first {np.flatnonzero(vref)[bad][:8]}"


@pytest.mark.parametrize("name", [c.name for c in W.CASES])
def test_wide_case_bit_for_bit(gpu, name):
    case = W.CASE[name]
    plan = TreePlan(W.doc(case.doc).compiled, gpu, **case.opts)
    W.assert_lowering(case, plan)  # with the split count of every launch below (launch_splits)
    X, Y, (ref, vref), (refy, vrefy) = W.reference(case.doc, case.rows)
    assert len(X) <= 600 and len(Y) <= 600
    Xt = torch.from_numpy(np.array(X)).to(gpu)
    for n in W.prefixes(case.rows):
        s, v, _ = _launch(plan, Xt[:n], case.launch)
        _same(f"{name} {n} rows", s, v, ref[:n], vref[:n])
    s, v, _ = _launch(plan, torch.from_numpy(np.array(Y)).to(gpu), case.launch)
    _same(f"{name} forced tiles", s, v, refy, vrefy)
    if plan.mode == 1:  # K-class chain: the softmax of exact integer logits, the bound PARITY.md states
        s, v, p = _launch(plan, Xt, case.launch, probs=True)
        _same(f"{name} with probs", s, v, ref, vref)
        _, vo, po = E.oracle(W.doc(case.doc).compiled, X)
        assert np.array_equal(vo, vref)
        r = np.abs(p[vref].astype(np.float64) - po[vref]).max() / 2.0 ** -24
        print(f"{name}: softmax ratio {r:.3f} x 2^-24")
        assert r <= E.C_BOUND["softmax"]


LAYOUTS = ("contiguous", "stride4", "odd", "offset4")


def _view(X, layout, gpu):
    """``X`` on the device: contiguous, or a column view of a wider matrix whose pad columns hold
    97.0 — row stride a multiple of 4 (vec4 loads with F % 4 != 0), odd, or a base 4 bytes off
    16-byte alignment over a stride that is a multiple of 4 (scalar loop by the pointer alone)."""
    F = X.shape[1]
    if layout == "contiguous":
        return torch.from_numpy(np.array(X)).to(gpu)
    if layout == "offset4":
        wide = np.full((X.shape[0], F + 4 + (-F) % 4), 97.0, F32)
        wide[:, 1:F + 1] = X
        t = torch.from_numpy(wide).to(gpu)[:, 1:F + 1]
        assert t.data_ptr() % 16 == 4 and t.stride(0) % 4 == 0
        return t
    extra = (4 - F % 4) if layout == "stride4" else (3 if (F + 3) % 2 else 4)
    t = torch.from_numpy(_exact.strided(np.array(X), extra)).to(gpu)[:, :F]
    if layout == "stride4":
        assert t.stride(0) % 4 == 0 and t.stride(0) > F and t.data_ptr() % 16 == 0
    else:
        assert t.stride(0) % 2 == 1
    return t


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("F", [5, 6, 7, 8])
def test_staging_loops_read_the_same_cells(gpu, F, layout):
    """The 19-tree SUM forest over F = 5..8 columns, all read: the float4 staging loop (identity
    map, 16-byte rows) and the scalar one give the oracle's bits whatever the row pitch."""
    name = "sum19" if F == 8 else f"sum19-f{F}"
    d = W.doc(name)
    plan = TreePlan(d.compiled, gpu, **W.WIDE)
    assert plan.variant & 3 == 1 and plan.mode == 0 and plan.rows_wide == 256 and plan.feat_map is None
    assert plan.n_stage == F
    X, Y, (ref, vref), (refy, vrefy) = W.reference(name, 256)
    for M, r, vr, what in ((X, ref, vref, "boundary"), (Y, refy, vrefy, "forced")):
        Xt = _view(M, layout, gpu)
        assert Xt.shape == M.shape
        s, v, _ = _launch(plan, Xt, dict(splits=1))
        _same(f"{name} {layout} {what}", s, v, r, vr)
