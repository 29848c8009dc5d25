"""GPU half of the derive-kernel probes: the ``[rows, n_sel]`` fp32 matrix ``derive.hip`` writes and its
``row_ok`` bytes against the row-at-a-time reference of tests/_derive_cases.py, bit for bit (NaN matches
NaN, the sign of zero counts), on every row of every column, at 1, 127, 128, 129 and 257 rows and the
full table, through ``DerivedPlan.launch`` and through a direct ``pmml_derive_launch`` on five input
layouts with guard elements around both outputs. The comparison is with the reference, not the twin."""

import numpy as np
import pytest

from tests import _derive_cases as D

CASES = {c: None for c in ("apply", "norm", "table", "chain", "fp32-column", "stack-16", "prep", "rounded", "wide-95",
                           "wide-96", "wide-256", "wide-96-one-selected")}
_PLANS = {}


def _case(name: str):
    if CASES[name] is None:
        CASES.update({c.name: c for c in D.plan_cases()})
    return CASES[name]


def _plan(name: str, gpu):
    from flink_jpmml_amd.runtime.derive import DerivedPlan

    if name not in _PLANS:
        plan = _case(name).c.plan(gpu)
        assert isinstance(plan, DerivedPlan)
        _PLANS[name] = plan
    return _PLANS[name]


def _assert_equal(case, cols: np.ndarray, row_ok: np.ndarray, n: int, what: str) -> None:
    ref = case.ref[:n]
    bad = ~D.same_bits(cols, ref)
    report = []
    for j in np.flatnonzero(bad.any(axis=0)):
        r = int(np.flatnonzero(bad[:, j])[0])
        report.append(f"{case.prog.selected[j]}: {int(bad[:, j].sum())} rows, e.g. row {r} input {case.X[r].tolist()} "
                      f"device {cols[r, j]!r} reference {ref[r, j]!r}")
    assert not report, f"{case.name} {what}:\n" + "\n".join(report)
    assert np.array_equal(row_ok, case.ok[:n].astype(np.uint8)), f"{case.name} {what}: row_ok"


def _launch(plan, X: np.ndarray, stream=None):
    import torch

    n = len(X)
    s = stream if stream is not None else torch.cuda.current_stream(plan.device)
    with torch.cuda.stream(s):
        Xt = torch.from_numpy(np.array(X, dtype=np.float32)).to(plan.device)  # a copy: the case's table is read-only
        sc, va = plan.alloc_outputs(n)
        Xa, ok = plan._buffers(stream, n)
        plan.launch(Xt, sc, va, stream=stream)
    s.synchronize()
    return Xa.cpu().numpy(), ok.cpu().numpy(), sc.cpu().numpy(), va.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", D.ROW_COUNTS + (0,), ids=lambda r: f"rows{r}" if r else "full")
@pytest.mark.parametrize("name", list(CASES))
def test_columns_and_row_ok(gpu, name, rows):
    case = _case(name)
    n = rows or len(case.X)
    cols, ok, score, valid = _launch(_plan(name, gpu), case.X[:n])
    _assert_equal(case, cols, ok, n, f"{n} rows")
    assert not valid[~case.ok[:n]].any() and np.isnan(score[~case.ok[:n]]).all()  # rejected rows score nothing


@pytest.mark.gpu
@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("name", ["apply", "prep"])
def test_direct_launch_layouts(gpu, name, layout):
    """The aligned float4 staging path (``ldx`` a multiple of 4, 16-byte base; ``n_in`` 6 and 3 are no
    multiples of 4), and the scalar path (odd ``ldx``, a base one float past the boundary; a contiguous
    matrix of 6 or 3 columns has ``ldx & 3 != 0`` too)."""
    case = _case(name)
    assert case.X.shape[1] % 4 != 0
    plan = _plan(name, gpu)
    for n in (129, len(case.X)):
        cols, ok, guards = D.launch_direct(plan, case.X[:n], layout)
        D.assert_guards(guards)
        _assert_equal(case, cols, ok, n, f"direct {layout} {n} rows")


@pytest.mark.gpu
def test_direct_launch_on_an_aligned_contiguous_matrix(gpu):
    """``n_in`` = 4: the contiguous matrix itself takes the float4 path."""
    case = _case("table")
    assert case.X.shape[1] == 4
    cols, ok, guards = D.launch_direct(_plan("table", gpu), case.X, "contiguous")
    D.assert_guards(guards)
    _assert_equal(case, cols, ok, len(case.X), "direct contiguous")


@pytest.mark.gpu
def test_non_default_stream(gpu):
    import torch

    s = torch.cuda.Stream(device=gpu)
    case = _case("apply")
    plan = _plan("apply", gpu)
    cols, ok, _, _ = _launch(plan, case.X, stream=s)
    _assert_equal(case, cols, ok, len(case.X), "plan launch on a side stream")
    case = _case("prep")
    cols, ok, guards = D.launch_direct(_plan("prep", gpu), case.X, "ldx-multiple-of-4", stream=s)
    D.assert_guards(guards)
    _assert_equal(case, cols, ok, len(case.X), "direct launch on a side stream")
