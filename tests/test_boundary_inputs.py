"""Inputs on the model's own boundaries (CPU): split thresholds, interval and outlier bounds,
sentinels, folded cuts, each +-2 fp32 ulps, and +-inf / NaN / +-0 / subnormal / +-FLT_MAX — the
inputs random draws never produce, and the ones on which "the fp32 comparison gives exactly the
fp64 answer for any fp32 input" (runtime/plans.py) can fail.

* ``emulate_prep``: a line-for-line numpy twin of ``common.h::prep_value`` over the words
  ``build_field_prep`` returns, against ``CompiledPmml.prepare`` on a grid of treatments
  (tests/_prep_grid.py): validity exact, values equal as fp32.
* every tree-layout emulator on ``boundary_matrix`` inputs against the oracle, bit for bit (integer
  leaves: any misrouted walk changes the sum), over operator pairs, child orders, fp32 and decimal
  thresholds, ``defaultChild`` and ``nullPrediction``.
* folded derived fields at every folded cut +-2 ulps and at +-inf.
* double inputs fp32 cannot hold: the device result is the oracle's on ``X.astype(float32)`` —
  inputs are rounded to nearest fp32, then every comparison is exact (docs/PARITY.md)."""

import numpy as np
import pytest
import torch

from tests import _boundary as B
from tests import _prep_grid as G

from flink_jpmml_amd.bench.synth import gbdt_pmml, random_forest_pmml
from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import TreePlan, build_field_prep, lowering_dry_run

F32 = np.float32


# --------------------------------------------------------------------------- prep_value twin


def emulate_prep(raw: np.ndarray, X32: np.ndarray) -> tuple:
    """``common.h::prep_value`` over ``build_field_prep``'s words, statement for statement, on an
    fp32 ``[rows, F]`` matrix: ``(prepared fp32, row rejected)``."""
    raw = np.ascontiguousarray(raw, dtype=np.uint32)
    words = raw.reshape(-1)
    fwords = words.view(F32)
    X32 = np.asarray(X32, dtype=F32)
    out = X32.copy()
    bad = np.zeros(len(X32), dtype=bool)
    for f in range(X32.shape[1]):
        fl = int(raw[f, 0])
        lo, hi, missing_repl, invalid_repl, out_lo, out_hi, pad = (F32(v) for v in raw[f, 1:8].view(F32))
        x = X32[:, f].copy()
        if fl == 0:
            continue
        if fl & PL.FP_ROW_INVALID:
            bad[:] = True
            continue
        with np.errstate(invalid="ignore"):
            miss = (x != x) | (bool(fl & PL.FP_MISSING_VALUE) & (x == pad))
            n_miss = n_inv = 0
            vlist = None
            if fl & PL.FP_VALUE_LIST:
                w = int(raw[f, 7])
                vlist = fwords[f * 8 + (w & 0xFFFF):]
                n_miss = (w >> 16) & 0xFF
                n_inv = w >> 24
                for i in range(n_miss):
                    miss = miss | (x == vlist[i])
            invalid = np.zeros(len(x), dtype=bool)
            for i in range(n_inv):
                invalid = invalid | (x == vlist[n_miss + i])
            if fl & PL.FP_HAS_INTERVAL:
                lo_ok = (x > lo) if fl & PL.FP_LO_OPEN else (x >= lo)
                hi_ok = (x < hi) if fl & PL.FP_HI_OPEN else (x <= hi)
                invalid = invalid | ~(lo_ok & hi_ok)
            if fl & PL.FP_CODE_RANGE:
                invalid = invalid | ~((x >= F32(0)) & (x < hi))
            if fl & PL.FP_INTEGER:
                invalid = invalid | (np.floor(x) != x)
            if fl & PL.FP_VALUE_MASK:
                d = x - lo
                inside = (d >= F32(0)) & (d < F32(64)) & (np.floor(x) == x)
                k = np.where(inside, d, 0).astype(np.int64)
                bits = np.where(k < 32, raw[f, 5], raw[f, 6]).astype(np.uint32)
                inside = inside & (((bits >> (k & 31).astype(np.uint32)) & 1) == 1)
                invalid = invalid | ~inside
            live = ~miss            # the `if (!miss)` block
            inv = live & invalid
            okv = live & ~invalid
            if fl & PL.FP_INVALID_RETURN:
                bad |= inv
            elif fl & PL.FP_INVALID_AS_MISSING:
                miss = miss | inv
            elif fl & PL.FP_INVALID_AS_VALUE:
                x = np.where(inv, invalid_repl, x)
            if fl & PL.FP_OUTLIER_AS_MISSING:
                miss = np.where(okv, (x < out_lo) | (x > out_hi), miss)
            elif fl & PL.FP_OUTLIER_AS_EXTREME:
                x = np.where(okv, np.minimum(np.maximum(x, out_lo), out_hi), x)
            x = np.where(miss, missing_repl if fl & PL.FP_HAS_MISSING_REPL else F32(np.nan), x)
        out[:, f] = x
    return out, bad


def _one_field_doc(case, dtype, ivt):
    _, children, data_type, attrs, _, _ = case
    return G.treat_field(gbdt_pmml(n_trees=1, depth=1, n_features=1, seed=0), 0, children, data_type, attrs, dtype, ivt)


GRID = G.grid()


@pytest.mark.parametrize("cell", GRID, ids=[g[0] for g in GRID])
def test_prep_twin_matches_oracle_on_the_bounds(cell):
    """Each treatment at its bounds +-{0, 1, 2} ulps, +-inf and NaN: the device's field preparation
    (its numpy twin over the lowered FieldPrep words) classifies and prepares every fp32 input as
    the fp64 oracle does."""
    _, case, dtype, ivt, _ = cell
    c = CompiledPmml.from_string(_one_field_doc(case, dtype, ivt))
    raw, any_prep = build_field_prep(c, c.active_fields)
    assert any_prep
    x = G.probe_values(case[4])
    X = x.reshape(-1, 1)
    ref, ok = c.prepare(X.astype(np.float64))
    got, bad = emulate_prep(raw, X)
    wrong = [(float(v), bool(o), bool(b)) for v, o, b in zip(x, ok, bad) if o == b]
    assert not wrong, f"validity differs (x, oracle valid, device rejected): {wrong}"
    a, b = got[ok, 0], ref[ok, 0].astype(F32)
    diff = [(float(v), float(p), float(q)) for v, p, q in zip(x[ok], a, b)
            if not (p == q or (np.isnan(p) and np.isnan(q)))]
    assert not diff, f"prepared value differs (x, device, oracle): {diff}"


def test_prep_twin_reads_value_lists_behind_the_pad_offset():
    """Several fields with lists: each record finds its own lists through the relative offset in
    its pad word (the second field's offset differs from the first's)."""
    txt = gbdt_pmml(n_trees=1, depth=2, n_features=3, seed=1)
    b = 0.3
    cases = G.families(b)["lists"]
    for j, k in enumerate((2, 0, 3)):
        _, children, data_type, attrs, _, _ = cases[k]
        txt = G.treat_field(txt, j, children, data_type, attrs, "double", "returnInvalid")
    c = CompiledPmml.from_string(txt)
    raw, _ = build_field_prep(c, c.active_fields)
    assert raw.shape[0] > 3  # list rows behind the three records
    vals = G.probe_values([G.SENT, -7.0, 0.5, 2.0, -1.0, b + 1])
    X = np.stack([np.roll(vals, s) for s in (0, 5, 11)], axis=1)
    ref, ok = c.prepare(X.astype(np.float64))
    got, bad = emulate_prep(raw, X)
    assert np.array_equal(ok, ~bad)
    np.testing.assert_array_equal(got[ok], ref[ok].astype(F32))


# --------------------------------------------------------------------------- tree layouts

N_TREES = 19
ROWS = 640


def _regression_doc(depth, F, mutant, missing="defaultChild", seed=5):
    txt = gbdt_pmml(n_trees=N_TREES, depth=depth, n_features=F, seed=seed, p_split=0.9 if depth <= 6 else 0.75)
    txt = B.integer_leaves(B.MUTANTS[mutant](txt))
    return B.null_prediction(txt) if missing == "nullPrediction" else txt


def _vote_doc(depth, F, mutant, missing="defaultChild", seed=6):
    txt = random_forest_pmml(n_trees=N_TREES, depth=depth, n_features=F, n_classes=3, seed=seed,
                             p_split=0.9 if depth <= 6 else 0.75)
    txt = B.integer_leaves(B.MUTANTS[mutant](txt), labels=("0", "1", "2"))
    return B.null_prediction(txt) if missing == "nullPrediction" else txt


def _case(txt, F, rows=ROWS, seed=1):
    c = CompiledPmml.from_string(txt)
    X = B.boundary_matrix(B.split_cuts(txt, F), rows, seed)
    ref, vref = c.score_matrix_oracle(X)
    return c, X, ref, vref


def _plan(c, **kw):
    with lowering_dry_run():
        return TreePlan(c, torch.device("cpu"), **kw)


def _affine(plan_or_spec, acc):
    e = plan_or_spec.epi_args if hasattr(plan_or_spec, "epi_args") else plan_or_spec.epi
    return e.get("a", 1.0) * np.asarray(acc, dtype=np.float64) + e.get("b", 0.0)


def _same(name, got, ref, vref):
    got = np.asarray(got, dtype=np.float64)
    assert np.array_equal(np.isfinite(got), vref), f"{name}: validity differs on {(np.isfinite(got) != vref).sum()} rows"
    bad = np.nonzero(got[vref].astype(F32) != ref[vref].astype(F32))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} of {vref.sum()} rows differ from the oracle"


def _wide_paths(name, plan, X, ref, vref):
    """Both tile paths of the wide kernel: with a NaN blob, a tile with a missing value takes the
    NaN blob over two planes (all rows go through it here), and the main blob only ever sees tiles
    without missing values (the rows without NaN go through it too)."""
    from test_wide_modes import emulate_wide

    if plan.blob_nan is None:
        _same(name, emulate_wide(plan, X, False), ref, vref)
        return
    _same(name + " NaN blob", emulate_wide(plan, X, True), ref, vref)
    stage = plan.feat_map.numpy() if plan.feat_map is not None else np.arange(X.shape[1])
    keep = ~np.isnan(X[:, stage]).any(axis=1)
    assert keep.sum() > len(X) // 4
    _same(name + " main blob", emulate_wide(plan, X[keep], False), ref[keep], vref[keep])


MISSING = ["defaultChild", "nullPrediction"]


@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("mutant", list(B.MUTANTS))
def test_perfect_layouts_bit_exact_on_thresholds(mutant, missing):
    """PERFECT narrow (``emulate_perfect``), its byte-address fast path with NaN planes
    (``emulate_perfect_fast``) and the wide kernel (``emulate_wide``, both tile paths), regression."""
    from test_lowering import _scores, emulate_perfect, emulate_perfect_fast
    from test_wide_modes import emulate_wide

    c, X, ref, vref = _case(_regression_doc(5, 8, mutant, missing), 8)
    B.assert_fp32_exact(ref, vref)
    assert vref.any() and (missing == "defaultChild" or not vref.all())
    spec, acc = emulate_perfect(c, X)
    _same("perfect", _scores(spec, acc), ref, vref)
    if missing == "defaultChild":
        _same("perfect fast + NaN planes", _affine(spec, emulate_perfect_fast(c, X, nan_planes=True)), ref, vref)
    plan = _plan(c)
    assert plan.layout == "perfect"
    _wide_paths("wide", plan, X, ref, vref)


@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("mutant", ["lt", "le-dec-rev"])
def test_perfect_vote_forest_labels_on_thresholds(mutant, missing):
    from test_lowering import _scores, emulate_perfect
    from test_wide_modes import emulate_wide

    c, X, ref, vref = _case(_vote_doc(5, 8, mutant, missing), 8)
    spec, acc = emulate_perfect(c, X)
    _same("perfect votes", _scores(spec, acc), ref, vref)
    plan = _plan(c)
    _wide_paths("wide votes", plan, X, ref, vref)


@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("mutant", list(B.MUTANTS))
def test_pointer_family_layouts_bit_exact_on_thresholds(mutant, missing):
    """Depth 9 (past the 5 LDS-staged LTOP levels, the hybrid head and the multi-level records):
    16-byte pointer, compact, super, LDS chunks, rank3 and both hybrid tails."""
    from test_hybrid_layout import emulate, emulate_super
    from test_lds_layout import emulate_lds
    from test_lowering import _scores, emulate_pointer
    from test_rank3 import walk_rank3

    from flink_jpmml_amd.runtime.hybrid import pack_rank3
    from flink_jpmml_amd.runtime.plans import ensemble_spec

    c, X, ref, vref = _case(_regression_doc(9, 8, mutant, missing), 8)
    B.assert_fp32_exact(ref, vref)
    assert vref.any()
    for name, kw in [("pointer wide", dict(layout="pointer", node_format="wide")),
                     ("pointer compact", dict(layout="pointer", node_format="compact")),
                     ("hybrid compact tail", dict(layout="hybrid")),
                     ("hybrid wide tail", dict(layout="hybrid", hybrid_tail="wide"))]:
        plan = _plan(c, **kw)
        _same(name, _affine(plan, emulate(plan, X)), ref, vref)
    plan = _plan(c, layout="pointer", node_format="super")
    _same("super", _affine(plan, emulate_super(plan, X)), ref, vref)
    plan = _plan(c, layout="pointer", node_format="lds")
    _same("lds", _affine(plan, emulate_lds(plan, X)), ref, vref)
    if missing == "defaultChild":  # these two walks model no null-on-missing flag
        spec, acc = emulate_pointer(c, X[:160])
        _same("pointer (per row)", _scores(spec, acc), ref[:160], vref[:160])
        spec = ensemble_spec(c)
        nodes, leaves, roots, thr, cnt, _ = pack_rank3(spec.trees, spec.weights, spec.P, c.n_features)
        _same("rank3", _affine(spec, walk_rank3(nodes, roots, thr, cnt, X)[:, 0]), ref, vref)


@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("mutant", ["lt", "le", "lt-rev", "le-dec-rev"])
def test_general_layout_bit_exact_on_thresholds(mutant, missing):
    from test_lowering import _scores

    from flink_jpmml_amd.runtime.general_tree import emulate_general, pack_general

    c, X, ref, vref = _case(_regression_doc(5, 8, mutant, missing), 8, rows=256)
    spec = PL.to_general(TreePlan._general_spec(c))
    packed = pack_general(spec.trees, spec.weights, spec.P, c.schema)
    acc = emulate_general(packed, X, spec.P, len(spec.trees))
    _same("general", _scores(spec, acc), ref, vref)


@pytest.mark.parametrize("dtype", ["double", "integer"])
def test_tree_layouts_on_double_and_integer_fields(dtype):
    """``dataType`` double (the oracle compares the unrounded fp64 constant) and integer (integer
    cuts; every non-integral neighbour is an invalid row) on the PERFECT and pointer walks."""
    from test_hybrid_layout import emulate
    from test_lowering import _scores, emulate_perfect

    txt = gbdt_pmml(n_trees=N_TREES, depth=5, n_features=8, seed=9)
    txt = B.integer_thresholds(txt) if dtype == "integer" else B.decimal_thresholds(txt)
    txt = B.integer_leaves(B.set_data_type(B.swap_operator_pair(txt), dtype))
    c = CompiledPmml.from_string(txt)
    if dtype == "integer":  # integer cuts everywhere; two rows of three carry one non-integral neighbour
        X = B.boundary_matrix(B.split_cuts(txt, 8), ROWS, 3, specials=False, ks=(0,))
        r = np.arange(ROWS)
        for k, sel in ((1, r % 3 == 1), (-1, r % 3 == 2)):
            X[r[sel], r[sel] % 8] = B.ulp_step(X[r[sel], r[sel] % 8], k)
    else:
        X = B.boundary_matrix(B.split_cuts(txt, 8), ROWS, 3)
    ref, vref = c.score_matrix_oracle(X)
    B.assert_fp32_exact(ref, vref)
    assert vref.any() and (dtype == "double" or not vref.all())
    raw, any_prep = build_field_prep(c, c.active_fields)
    P, bad = emulate_prep(raw, X) if any_prep else (X, np.zeros(len(X), bool))
    assert np.array_equal(~bad, vref)
    spec, acc = emulate_perfect(c, P)
    _same("perfect", np.where(bad, np.nan, _scores(spec, acc)), ref, vref)
    plan = _plan(c, layout="pointer", node_format="wide")
    _same("pointer", np.where(bad, np.nan, _affine(plan, emulate(plan, P))), ref, vref)


# --------------------------------------------------------------------------- folded derived fields


def folded_case(n_trees=N_TREES, depth=5, F=8, seed=11, rows=ROWS):
    """``gbdt_pmml(scaled=True)`` with integer leaves, and inputs at every folded cut +-2 ulps plus
    the special values (+-inf among them)."""
    from flink_jpmml_amd.runtime.derive import plan_field_layout

    txt = B.integer_leaves(gbdt_pmml(n_trees=n_trees, depth=depth, n_features=F, scaled=True, seed=seed))
    c = CompiledPmml.from_string(txt)
    layout = plan_field_layout(c, allow_fold=True)
    assert layout.program is None and len(layout.folds) == F
    cuts = [[] for _ in range(F)]
    for name, (src, _, memo) in layout.folds.items():
        j = c.active_fields.index(src)
        cuts[j] += [t for _, t in memo.values() if np.isfinite(t)] or [0.0]
    X = B.boundary_matrix(cuts, rows, seed)
    return txt, c, X


def test_folded_fields_at_their_cuts_and_at_infinity():
    """Monotone derived fields folded into thresholds on the raw input: exact at every folded cut
    +-2 ulps and at +-inf. (An always-true fold written ``x < +inf`` misroutes ``x = +inf``, which
    the oracle accepts as a value of a clamped ``NormContinuous``.)"""
    from test_wide_modes import emulate_wide

    from flink_jpmml_amd.runtime.plans import compile_plan

    txt, c, X = folded_case()
    ref, vref = c.score_matrix_oracle(X)
    B.assert_fp32_exact(ref, vref)
    with lowering_dry_run():
        plan = compile_plan(c, torch.device("cpu"))
    assert type(plan).__name__ == "TreePlan" and plan.layout == "perfect"
    _wide_paths("folded wide", plan, X, ref, vref)
    # one column at +inf / -inf at a time: every constant fold on that column is exercised
    base = B.boundary_matrix([[0.0]] * 8, 64, 0, specials=False)
    for value in (np.inf, -np.inf):
        for j in range(8):
            Xi = base.copy()
            Xi[:, j] = value
            Xi[:, (j + 1) % 8] = X[:64, (j + 1) % 8]
            r, v = c.score_matrix_oracle(Xi)
            _wide_paths(f"f{j} = {value}", plan, Xi, r, v)


def test_constant_folds_keep_their_value_at_infinity_and_nan_takes_the_default():
    from flink_jpmml_amd.models.tree import OP_GE, OP_GT, OP_LE, OP_LT
    from flink_jpmml_amd.runtime.derive import fold_splits
    from flink_jpmml_amd.runtime.plans import canonical_threshold

    f = lambda x: np.clip(x, -1.0, 1.0)  # noqa: E731 - a clamped NormContinuous
    xs = np.array([-np.inf, -B.FLT_MAX, -1.0, 0.0, 1.0, B.FLT_MAX, np.inf])
    for op, t in [(OP_LT, 5.0), (OP_LE, 1.0), (OP_GT, -5.0), (OP_GE, -1.0), (OP_LT, -5.0), (OP_GT, 5.0),
                  (OP_GE, 1.5), (OP_LE, -1.5), (OP_LT, 0.25), (OP_GE, 0.25)]:
        o2, t2 = fold_splits(f, np.array([op], np.int8), np.array([t]))
        y = f(xs)
        want = {OP_LT: y < t, OP_LE: y <= t, OP_GT: y > t, OP_GE: y >= t}[op]
        T, swap = canonical_threshold(int(o2[0]), float(t2[0]))
        right = xs.astype(F32) >= F32(T)
        assert np.array_equal(right if swap else ~right, want), (op, t, o2, t2)
        # NaN: `x >= T` is false whatever T, so the kernels route it by the node's default bit, and
        # the NaN-plane fast path (NaN -> +inf on default-right nodes) sends it right for every T
        assert not (F32(np.nan) >= F32(T)) and F32(np.inf) >= F32(T)


# --------------------------------------------------------------------------- doubles fp32 cannot hold


def test_double_inputs_round_to_nearest_fp32_then_compare_exactly():
    """The known deviation, pinned: a double input fp32 cannot hold (0.8 on a ``double`` field under
    ``lessOrEqual 0.8``) is rounded to the nearest fp32, and the device result is exactly the
    oracle's on that fp32 value — not the oracle's on the double."""
    from test_hybrid_layout import emulate
    from test_lowering import _scores, emulate_perfect

    txt = gbdt_pmml(n_trees=N_TREES, depth=5, n_features=8, seed=13)
    txt = B.rewrite_thresholds(txt, lambda t: f"{t:.1f}")
    txt = B.integer_leaves(B.set_data_type(B.swap_operator_pair(txt), "double"))
    c = CompiledPmml.from_string(txt)
    cuts = B.split_cuts(txt, 8)
    rng = np.random.default_rng(0)
    X = np.stack([rng.choice(np.asarray(cu), ROWS) for cu in cuts], axis=1)  # one-decimal doubles
    assert (X.astype(F32).astype(np.float64) != X).any()
    ref32, v32 = c.score_matrix_oracle(X.astype(F32))
    B.assert_fp32_exact(ref32, v32)
    spec, acc = emulate_perfect(c, X)
    _same("perfect", _scores(spec, acc), ref32, v32)
    plan = _plan(c, layout="pointer", node_format="wide")
    _same("pointer", _affine(plan, emulate(plan, X)), ref32, v32)
    ref64, _ = c.score_matrix_oracle(X)
    assert not np.array_equal(ref64, ref32)  # the deviation is real: fp32(0.8) > 0.8
