"""CPU half of the derive-kernel probes (tests/_derive_cases.py): the tables hold what they claim, the
exactness guard and the 2^-40 midpoint condition hold on the final tables, the row-at-a-time
reference equals the float64 oracle and the numpy twin on every row of every column, the restated
twin equals ``runtime/derive.py::emulate`` and every named mutant of it shows, and the lowering's two
limits (stack depth 16, 256 tile columns) hold. tests/test_gpu_derive.py compares the kernel with the
same reference."""

import warnings

import numpy as np
import pytest

from tests import _derive_cases as D

from flink_jpmml_amd.runtime.plans import NotLowerable

CASES = {"apply": D.apply_case, "norm": D.norm_case, "table": D.table_case, "chain": D.chain_case,
         "stack-16": D.stack_case, "prep": D.prep_case, "rounded": D.rounded_case, "wide-95": lambda: D.wide_case(95),
         "wide-96": lambda: D.wide_case(96), "wide-256": lambda: D.wide_case(256),
         "wide-96-one-selected": D.n_sel_one_case}


def _differences(case, got: np.ndarray) -> list:
    bad = ~D.same_bits(got, case.ref)
    out = []
    for j in np.flatnonzero(bad.any(axis=0)):
        r = int(np.flatnonzero(bad[:, j])[0])
        out.append((case.prog.selected[j], int(bad[:, j].sum()), case.X[r].tolist(), float(got[r, j]), float(case.ref[r, j])))
    return out


def test_plan_cases_lists_every_case():
    assert {c.name for c in D.plan_cases()} == set(CASES) | {"fp32-column"}
    for c in D.plan_cases():
        assert max(D.ROW_COUNTS) < len(c.X) <= 1025, (c.name, len(c.X))  # every row count is a real prefix


@pytest.mark.parametrize("name", ["apply", "norm", "table", "chain", "prep", "rounded"])
def test_every_population_is_placed(name):
    case = CASES[name]()
    assert case.claims
    empty = [k for k, rows in case.claims.items() if not np.any(rows)]
    assert not empty, empty


@pytest.mark.parametrize("name", [n for n in CASES if n != "rounded"])
def test_exact_family_guard(name):
    """No float64 intermediate of the final table is inexact and no column that another field reads
    holds a rounded fp32 value. Stored values that fp32 rounds are leaves, and are the store cases."""
    case = CASES[name]()
    print(f"{name}: {len(case.X)} rows, {case.dropped} dropped by the builder")
    assert not case.inexact.any()
    assert not case.inexact_read
    assert case.dropped <= 64
    if name == "apply":
        rounded = {k for k, rows in case.rounded_store.items() if rows}
        assert {"over", "under"} <= rounded


def test_no_rounded_probe_is_near_a_midpoint():
    case = D.rounded_case()
    m = case.margins
    assert len(m) > 4000
    assert int((m <= D.MID_REL).sum()) == 0
    print(f"{len(m)} evaluations, {int(np.isinf(m).sum())} fixed by C99 or exact, smallest margin 2^{np.log2(m.min()):.1f}")
    # the condition is not vacuous: the probe it replaced in the first table
    assert D.rounded_value("sqrt", D.BIG_INT)[1] < D.MID_REL
    assert not (case.X[:, 0] == D.BIG_INT).any()


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_oracle(name):
    case = CASES[name]()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # np.nanmin of an all-missing row
        got = case.oracle()
    assert not _differences(case, got)
    P, ok = case.c.prepare(case.X.astype(np.float64))
    assert np.array_equal(P, case.P, equal_nan=True) and np.array_equal(ok, case.ok)


@pytest.mark.parametrize("name", list(CASES) + ["fp32-column"])
def test_reference_equals_twin_and_twin_equals_emulate(name):
    from flink_jpmml_amd.runtime.derive import emulate

    case = D.fp32_column_case() if name == "fp32-column" else CASES[name]()
    cols, row_ok = case.twin()
    assert not _differences(case, cols)
    assert np.array_equal(row_ok, case.ok.astype(np.uint8))
    assert D.same_bits(cols, emulate(case.prog, case.P)).all()


def test_fp32_columns_between_chained_fields():
    """``d1 = a / 3`` is a ``double`` field, but the tile holds fp32 columns: ``d2 = greaterThan(d1 * 3, a)``
    reads ``fp32(d1)`` on the device and in the twin, the float64 ``d1`` in the oracle (docs/PARITY.md,
    deliberate deviations). The reference evaluates either rule; each side equals its own on every
    row, and the rows on which the two rules part are a known, non-empty set."""
    case = D.fp32_column_case()
    ref64 = D.Reference(case.c, fp32_columns=False).columns(case.P, case.prog.selected)
    assert D.same_bits(case.oracle(), ref64).all()
    assert D.same_bits(case.twin()[0], case.ref).all()
    j = case.prog.selected.index("d2")
    part = ~D.same_bits(ref64[:, j], case.ref[:, j])
    a = case.X[:, 0].astype(np.float64)
    third = (a / 3.0).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        expect = np.isfinite(a) & ((third * 3.0 > a) != ((a / 3.0) * 3.0 > a))
    assert np.array_equal(part, expect) and 50 < part.sum() < len(a)
    assert (ref64[~np.isnan(a), j] == 0).all()  # in float64, (a / 3) * 3 never exceeds these a


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_every_mutant_shows(mutant):
    shown = []
    for case in D.plan_cases():
        cols, row_ok = case.twin(mutant)
        if not D.same_bits(cols, case.ref).all() or not np.array_equal(row_ok, case.ok.astype(np.uint8)):
            shown.append(case.name)
    print(f"{mutant}: {shown}")
    assert bool(shown) == (mutant not in D.INERT_MUTANTS)


def test_stack_depth_limit():
    from flink_jpmml_amd.runtime.compiled import CompiledPmml
    from flink_jpmml_amd.runtime.derive import STACK_DEPTH, plan_field_layout

    assert STACK_DEPTH == 16 and D.stack_case().prog.max_stack == 16
    with pytest.raises(NotLowerable):
        plan_field_layout(CompiledPmml.from_string(D.stack_document(17)))


def test_tile_column_limits():
    from flink_jpmml_amd.runtime.compiled import CompiledPmml
    from flink_jpmml_amd.runtime.derive import plan_field_layout

    def lds(n_tile):
        return 16384 + 512 * n_tile + 512

    assert lds(95) <= 65536 < lds(96) and lds(256) <= 160 * 1024
    for n_tile in (95, 96):
        prog = D.wide_case(n_tile).prog
        assert prog.n_tile == n_tile == len(prog.selected)
    prog = D.wide_case(256).prog  # the regression kernel behind the derive pass reads 128 columns at most
    assert prog.n_tile == 256 and len(prog.selected) == 128
    one = D.n_sel_one_case().prog
    assert one.n_tile == 96 and len(one.selected) == 1
    with pytest.raises(NotLowerable):
        plan_field_layout(CompiledPmml.from_string(D.wide_document(257)))


def test_every_document_lowers_to_a_derived_plan():
    """What tests/test_gpu_derive.py launches: a ``DerivedPlan`` carrying the program the cases emulate."""
    from flink_jpmml_amd.runtime.derive import DerivedPlan
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    with lowering_dry_run():
        for case in D.plan_cases():
            plan = case.c.plan("cpu")
            assert isinstance(plan, DerivedPlan), case.name
            assert (plan.n_tile, plan.n_sel) == (case.prog.n_tile, len(case.prog.selected))
            assert plan.program.insns.tobytes() == case.prog.insns.tobytes()  # bytes: NaN operands compare too
            assert plan.program.pool.tobytes() == case.prog.pool.tobytes()


def test_layouts_of_the_direct_harness():
    X = np.arange(5 * 6, dtype=np.float32).reshape(5, 6)
    seen = {}
    for layout in D.LAYOUTS:
        buf, off, ldx = D.lay_out(X, layout)
        rows = np.stack([buf[off + r * ldx: off + r * ldx + 6] for r in range(5)])
        assert np.array_equal(rows, X)
        assert (np.delete(buf, [off + r * ldx + j for r in range(5) for j in range(6)]) == 97).all()
        assert off + 4 * ldx + (6 + 3) // 4 * 4 <= len(buf)  # the last row's float4 loads stay inside
        seen[layout] = (off, ldx)
    assert seen["contiguous"] == (0, 6)
    assert seen["ldx-multiple-of-4"][1] % 4 == 0 and seen["ldx-multiple-of-4"][1] > 6
    assert seen["odd-ldx"][1] % 2 == 1 and seen["odd-ldx"][1] > 6
    assert seen["misaligned-base"][0] == 1 and seen["misaligned-base"][1] % 4 == 0


def test_normal_cdf_lower_tail_of_the_oracle():
    """``stdNormalCDF`` and the host-only ``normalCDF`` in the erfc form: no cancellation below -8."""
    import mpmath

    from flink_jpmml_amd.pmml.fields import _TERNARY_NUM, _UNARY_NUM

    mpmath.mp.prec = 200
    for a in (-1.0, -4.0, -6.0, -8.0, -8.5, -10.0, -13.0, 0.0, 8.5):
        true = float(mpmath.ncdf(a))
        assert abs(float(_UNARY_NUM["stdNormalCDF"](np.float64(a))) - true) <= 1e-14 * true
        got = float(_TERNARY_NUM["normalCDF"](np.float64(2.0 * a + 1.0), np.float64(1.0), np.float64(2.0)))
        assert abs(got - true) <= 1e-14 * true
