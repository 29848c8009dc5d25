"""Scorecard documents whose reason-code situations are placed by construction, an independent
row-at-a-time reference, and named mutants of the numpy twin (``ops/reasons.py``).

Every characteristic of a case is a selector: attribute ``k`` matches ``f_j == k``, so an input row of
small integers names the attribute each characteristic takes; a missing value makes every predicate
UNKNOWN and a value outside the bins matches nothing (the characteristic stays unmatched and the
score is missing). Partial scores and baselines are chosen so that the differences tie, round, cancel
or reorder exactly where the case says.
"""

import contextlib
import itertools
import math

import numpy as np

from flink_jpmml_amd.bench.synth import reason_scorecard_pmml

NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# --------------------------------------------------------------------------- document builders


def eq(j, v):
    return f'<SimplePredicate field="f{j}" operator="equal" value="{v}"/>'


def missing(j):
    return f'<SimplePredicate field="f{j}" operator="isMissing"/>'


def selector(j, partials, codes=None, code=None, baseline=None, complex_=None):
    """Characteristic ``j``: attribute ``k`` matches ``f_j == k`` with ``partials[k]``."""
    attrs = []
    for k, p in enumerate(partials):
        a = {"predicate": eq(j, k), "partial": p}
        if codes is not None and codes[k] is not None:
            a["reason_code"] = codes[k]
        if complex_ is not None and k in complex_:
            a["complex"] = complex_[k][0]
            a["partial"] = None
        attrs.append(a)
    return {"name": f"ch{j}", "reason_code": code, "baseline": baseline, "attributes": attrs}


def grid(*levels):
    """Every combination of the given per-field values, as fp32 rows."""
    return np.array(list(itertools.product(*levels)), dtype=np.float32)


def _case(name, chars, X, what, **kw):
    kw.setdefault("n_features", X.shape[1])
    return {"name": name, "chars": chars, "X": np.ascontiguousarray(X, dtype=np.float32), "what": what, "kw": kw}


def document(case, strip_char_baselines=False):
    chars = case["chars"]
    if strip_char_baselines:
        chars = [dict(c, baseline=None) for c in chars]
    return reason_scorecard_pmml(chars, **case["kw"])


def _cases():
    out = []
    # differences {3, 5, 0, -2} in three characteristics with their own codes: equal differences keep
    # characteristic order; zero and negative differences rank below; NaN / 9 leave one unmatched
    lv = (0, 1, 2, 3, NAN, 9)
    out.append(_case("equal_diffs", [selector(j, [7, 5, 10, 12], code=c) for j, c in enumerate("CBA")],
                     grid(lv, lv, (0, 1, 2, 3)), "disjoint, K=4", ranks=(1, 2, 3), baseline=10.0))
    # S belongs to ch0 and ch2, T to ch1: S = d0 + d2 ties with T = d1 on (1+1 | 2), (1+2 | 3), (2+2 | 4)
    out.append(_case("shared_tie", [selector(0, [9, 8], code="S"), selector(1, [8, 7, 6], code="T"),
                                    selector(2, [9, 8], code="S")],
                     grid((0, 1), (0, 1, 2), (0, 1, NAN)), "shared, K=4", ranks=(1, 2, 3), baseline=10.0))
    # attribute-level codes: Z then A in the document, but row (1, 1) touches A first; equal differences
    out.append(_case("flip_touch", [selector(0, [9, 9], codes=["Z", "A"]), selector(1, [9, 9], codes=["A", "Z"]),
                                    selector(2, [9, 9.5], codes=["Q", "Z"])],
                     grid((0, 1), (0, 1), (0, 1)), "shared, K=2", ranks=(1, 2), baseline=10.0))
    # -0.0 (baseline -0.0 minus partial 0.0) against +0.0: equal, so characteristic order
    out.append(_case("signed_zero", [selector(0, [0.0, 1.0], code="A", baseline=-0.0),
                                     selector(1, [0.0, -1.0], code="B", baseline=0.0),
                                     selector(2, [0.0], code="C", baseline=-0.0)],
                     grid((0, 1), (0, 1), (0,)), "disjoint, K=1", ranks=(1,), baseline=5.0))
    # 2^24 against 2^24 + 1: equal after fp32 rounding, B first in float64
    out.append(_case("fp32_rounding", [selector(0, [-2.0 ** 24, -1.0], code="A"),
                                       selector(1, [-(2.0 ** 24 + 1), -2.0], code="B")],
                     grid((0, 1), (0, 1)), "disjoint, K=2", ranks=(1, 2), baseline=0.0))
    # (1e16 + 1) + 1 = 1e16 in characteristic order, 1 + 1 + 1e16 = 1e16 + 2 = T in another order
    out.append(_case("order3", [selector(0, [-1e16], code="S"), selector(1, [-1.0, 0.0], code="S"),
                                selector(2, [-1.0, 0.0], code="S"), selector(3, [-(1e16 + 2)], code="T")],
                     grid((0,), (0, 1), (0, 1), (0,)), "shared, K=1", ranks=(1,), baseline=0.0))
    # attributes and characteristics without a code; fewer codes than the requested rank
    out.append(_case("no_codes", [selector(0, [1, 2], codes=["X", None]), selector(1, [3, 4]),
                                  selector(2, [5, 20], code="C")],
                     grid((0, 1), (0, 1), (0, 1)), "disjoint, K=4", ranks=(1, 2, 3), baseline=10.0))
    # pointsAbove: partial - baseline
    out.append(_case("points_above", [selector(0, [12, 15], code="A"), selector(1, [14, 11], code="B"),
                                      selector(2, [13, 9], code="A")],
                     grid((0, 1), (0, 1), (0, 1)), "shared, K=2", ranks=(1, 2), baseline=10.0,
                     algorithm="pointsAbove"))
    # ch1's own baseline 20 puts B first; with the model's 10 it would come last
    out.append(_case("char_baseline", [selector(0, [7, 8], code="A"), selector(1, [9, 12], code="B", baseline=20.0),
                                       selector(2, [6, 9.5], code="C")],
                     grid((0, 1), (0, 1), (0, 1)), "disjoint, K=2", ranks=(1, 2), baseline=10.0))
    # useReasonCodes="false": NaN columns
    out.append(_case("use_false", [selector(0, [7, 8], code="A"), selector(1, [9, 12], code="B")],
                     grid((0, 1), (0, 1, NAN)), "no kernel", ranks=(1, 2), baseline=10.0, use_reason_codes=False))
    # MiningField preparation: f0 outside [0, 1] fails the row (2 has an attribute); a missing f1 is replaced by 1; a
    # characteristic whose first attribute is UNKNOWN on a missing value while a later one is TRUE
    out.append(_case("prep", [selector(0, [7, 8, 6], code="A"), selector(1, [9, 6], code="B"),
                              {"name": "ch2", "reason_code": "C", "baseline": None, "attributes": [
                                  {"predicate": eq(2, 0), "partial": 1.0},
                                  {"predicate": f'<CompoundPredicate booleanOperator="or">{missing(2)}{eq(2, 1)}'
                                                '</CompoundPredicate>', "partial": 9.5, "reason_code": "M"},
                                  {"predicate": '<CompoundPredicate booleanOperator="surrogate">'
                                                f'{eq(2, 2)}<True/></CompoundPredicate>', "partial": 4.0},
                                  {"predicate": '<SimpleSetPredicate field="f2" booleanOperator="isIn">'
                                                '<Array n="2" type="real">3 4</Array></SimpleSetPredicate>',
                                   "partial": 8.5, "reason_code": "S"}]}],
                     grid((0, 1, 2, -1), (0, 1, NAN), (0, 1, 2, 3, 4, NAN, 9)), "disjoint, K=4", ranks=(1, 2, 3),
                     baseline=10.0, intervals={0: (0.0, 1.0)}, mining={1: 'missingValueReplacement="1"'}))
    # ComplexPartialScore: 0.5 * f2 and f2 - 2 on the 1/8 grid are exact fp32 numbers
    half = ('<Apply function="*"><FieldRef field="f2"/><Constant dataType="double">0.5</Constant></Apply>',
            lambda r: 0.5 * r[2])
    minus = ('<Apply function="-"><FieldRef field="f2"/><Constant dataType="double">2</Constant></Apply>',
             lambda r: r[2] - 2.0)
    eighths = (0.0, 0.125, 1.5, 3.875, 6.0, 8.25, -4.5, NAN)
    for name, algo in (("complex", "pointsBelow"), ("complex_above", "pointsAbove")):
        out.append(_case(name, [selector(0, [None, 3.0], codes=["A", "A2"], complex_={0: half}),
                                selector(1, [2.0, None], code="B", complex_={1: minus}),
                                selector(3, [1.0, 3.5], code="A")],
                         grid((0, 1), (0, 1), eighths, (0, 1)), "shared, K=2, derive tile", ranks=(1, 2), baseline=4.0,
                         algorithm=algo))
    # 64 codes (8 characteristics x 8 attribute codes), ranks 1 .. 8
    rng = np.random.default_rng(64)
    X8 = rng.integers(0, 8, (300, 8)).astype(np.float32)
    part = rng.integers(0, 6, (8, 8)).astype(np.float64)  # many equal differences
    out.append(_case("codes64", [selector(j, list(part[j]), codes=[f"c{j}_{k}" for k in range(8)]) for j in range(8)],
                     X8, "disjoint, K=8", ranks=tuple(range(1, 9)), baseline=3.0))
    shared = [[f"c{j}_{k}" for k in range(8)] for j in range(8)]
    for j in range(1, 8):
        shared[j][0] = "c0_0"  # one code in every characteristic: 57 codes ...
    chars = [selector(j, list(part[j]), codes=shared[j]) for j in range(8)]
    chars.append(selector(8, [1.0] * 7, codes=[f"x{k}" for k in range(7)]))  # ... and 7 more: 64
    X9 = np.concatenate([X8, rng.integers(0, 7, (300, 1)).astype(np.float32)], axis=1)
    out.append(_case("codes64_shared", chars, X9, "shared, K=8, 64 rows per workgroup", ranks=tuple(range(1, 9)),
                     baseline=3.0))
    return out


CASES = _cases()
CASE = {c["name"]: c for c in CASES}


def too_many_codes():
    """65 codes: ``codes64`` plus one attribute."""
    c = CASE["codes64"]
    chars = [dict(ch) for ch in c["chars"]]
    chars[0] = dict(chars[0], attributes=chars[0]["attributes"] + [{"predicate": eq(0, 8), "partial": 1.0,
                                                                    "reason_code": "one_more"}])
    return reason_scorecard_pmml(chars, **c["kw"])


def with_ranks(name, ranks):
    c = CASE[name]
    return reason_scorecard_pmml(c["chars"], **dict(c["kw"], ranks=ranks))


def no_baseline():
    c = CASE["char_baseline"]
    return reason_scorecard_pmml(c["chars"], **dict(c["kw"], baseline=None))


# --------------------------------------------------------------------------- reference


def _pred(p, row):
    """Three-valued value (True / False / None) of an ``ir`` predicate on a prepared row."""
    from flink_jpmml_amd.pmml import ir

    if isinstance(p, ir.TruePredicate):
        return True
    if isinstance(p, ir.FalsePredicate):
        return False
    if isinstance(p, ir.SimplePredicate):
        x = row[int(p.field[1:])]
        if p.operator == "isMissing":
            return math.isnan(x)
        if p.operator == "isNotMissing":
            return not math.isnan(x)
        if math.isnan(x):
            return None
        v = float(p.value)
        return {"equal": x == v, "notEqual": x != v, "lessThan": x < v, "lessOrEqual": x <= v,
                "greaterThan": x > v, "greaterOrEqual": x >= v}[p.operator]
    if isinstance(p, ir.SimpleSetPredicate):
        x = row[int(p.field[1:])]
        if math.isnan(x):
            return None
        inside = any(x == float(v) for v in p.values)
        return inside if p.boolean_operator == "isIn" else not inside
    vals = [_pred(q, row) for q in p.predicates]
    op = p.boolean_operator
    if op == "and":
        return False if False in vals else (None if None in vals else True)
    if op == "or":
        return True if True in vals else (None if None in vals else False)
    if op == "xor":
        return None if None in vals else (sum(vals) % 2 == 1)
    return next((v for v in vals if v is not None), None)  # surrogate


def reference(case, compiled):
    """Row at a time from the parsed document: ``(codes per row, valid per row)``. A row is valid when
    its preparation passes, every characteristic matches and every picked expression has a value."""
    sc = compiled.model
    P, ok = compiled.prepare(case["X"])
    fns = {}
    for ch in case["chars"]:
        for k, a in enumerate(ch["attributes"]):
            if a.get("complex"):
                fns[(ch["name"], k)] = next(f for xml, f in _complex_fns() if xml == a["complex"])
    out, valid = [], []
    for r in range(len(P)):
        row = [float(v) for v in P[r]]
        acc, good = {}, bool(ok[r])
        for ch in sc.characteristics:
            base = ch.baseline_score if ch.baseline_score is not None else sc.baseline_score
            pick = next((k for k, a in enumerate(ch.attributes) if _pred(a.predicate, row) is True), None)
            if pick is None:
                good = False
                continue
            a = ch.attributes[pick]
            partial = fns[(ch.name, pick)](row) if a.complex_score is not None else a.partial_score
            if math.isnan(partial):
                good = False
            code = a.reason_code or ch.reason_code
            if code is None:
                continue
            d = (base - partial) if sc.reason_code_algorithm == "pointsBelow" else (partial - base)
            acc[code] = acc.get(code, 0.0) + d
        order = []
        left = list(acc.items())
        while left:  # repeated selection of the largest sum, the earliest on ties
            best = 0
            for i in range(1, len(left)):
                if left[i][1] > left[best][1]:
                    best = i
            order.append(left.pop(best)[0])
        out.append(order)
        valid.append(good)
    return out, np.array(valid, dtype=bool)


def _complex_fns():
    return [('<Apply function="*"><FieldRef field="f2"/><Constant dataType="double">0.5</Constant></Apply>',
             lambda r: 0.5 * r[2]),
            ('<Apply function="-"><FieldRef field="f2"/><Constant dataType="double">2</Constant></Apply>',
             lambda r: r[2] - 2.0)]


def expected_matrix(case, compiled, codes, valid):
    """The fp32 output matrix the reference implies: ``schema.lookup`` of the ranked code, NaN on
    invalid rows and past the row's codes (and everywhere with ``useReasonCodes="false"``)."""
    fields = list(compiled.model.output)
    out = np.full((len(codes), len(fields)), np.nan, dtype=np.float32)
    if not compiled.model.use_reason_codes:
        return out
    for j, of in enumerate(fields):
        k = int(of.rank) - 1
        for r, row in enumerate(codes):
            if valid[r] and len(row) > k:
                out[r, j] = compiled.schema.lookup(of.name, row[k])
    return out


# --------------------------------------------------------------------------- the twin and its mutants


def dry_plan(text):
    """``(compiled, output plan)`` lowered on the host with ``reason_codes=True``."""
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    compiled = PmmlModel.from_string(text).compiled
    with lowering_dry_run():
        return compiled, compiled.output_plan("cpu", reason_codes=True)


def kernel_inputs(plan, X):
    """What the reason kernel reads for the raw rows ``X``: ``(matrix fp32, valid uint8, FieldPrep
    table or None)``, from the plan's dry run."""
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    with lowering_dry_run():
        _, v, _ = plan.score_outputs(X)
    prep = plan._reason_prep.numpy() if plan._reason_prep is not None else None
    Xr = np.ascontiguousarray(plan._reason_matrix_host(np.asarray(X, dtype=np.float32)), dtype=np.float32)
    return Xr, np.asarray(v.numpy() if hasattr(v, "numpy") else v, dtype=np.uint8), prep


def twin(plan, X, tables=None, rows=None):
    from flink_jpmml_amd.ops.reasons import reasons_numpy

    Xr, valid, prep = kernel_inputs(plan, X)
    T = tables if tables is not None else plan.reasons
    out = np.full((len(Xr), T.width), 7.0, dtype=np.float32)
    return reasons_numpy(Xr, valid, out, T, prep=prep, rows=rows)


def retabled(T, **over):
    from flink_jpmml_amd.ops.reasons import ReasonTables

    kw = dict(chars=T.chars, attrs=T.attrs, dval=T.dval, preds=T.preds, pool=T.pool, cols=T.cols, tables=T.tables,
              n_code=T.n_code, n_feat=T.n_feat, width=T.width, above=T.above, shared=T.shared)
    kw.update(over)
    return ReasonTables(**kw)


@contextlib.contextmanager
def _patched(name, value):
    from flink_jpmml_amd.ops import reasons as R

    old = getattr(R, name)
    setattr(R, name, value)
    try:
        yield
    finally:
        setattr(R, name, old)


def _rule(name, value):
    def run(case, plan):
        with _patched(name, value):
            return twin(plan, case["X"])
    return run


def _no_merge(case, plan):
    return twin(plan, case["X"], retabled(plan.reasons, shared=False))


def _wrong_sign(case, plan):
    T = plan.reasons
    if not T.above:
        return twin(plan, case["X"])
    return twin(plan, case["X"], retabled(T, dval=np.where(T.attrs[:, 2] < 0, -T.dval, T.dval), above=False))


def _model_baseline(case, plan):
    _, other = dry_plan(document(case, strip_char_baselines=True))
    return twin(other, case["X"])


def _ge(p, v):
    with np.errstate(invalid="ignore"):
        return p >= v


MUTANTS = {
    "fp32 accumulation": _rule("_ACC", np.float32),
    "ties to the lower code index": _rule("_tie", lambda t, bt: np.zeros(len(t), dtype=bool)),
    "non-strict compare": _rule("_beats", _ge),
    "no merging of a shared code": _no_merge,
    "wrong sign for pointsAbove": _wrong_sign,
    "model baseline for a characteristic with its own": _model_baseline,
    "UNKNOWN treated as a match": _rule("_match", lambda v: v != 0),
}
