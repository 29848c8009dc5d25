"""Prescribed per-segment results for the segment-reduction kernel (``ops/csrc/segment.hip``), its
torch twin (``runtime/segmented.py``) and the float64 oracle (``models/mining.py``).

A :class:`Case` is a document of K one-leaf tree segments (segment i applies where ``f<i> > 0``)
plus one row-indexed table: the input matrix ``X`` (1 = TRUE, -1 = FALSE, NaN = UNKNOWN; both
non-applying spellings occur in every grid), the segment scores ``S[K, n]``, their validity
``V[K, n]`` and, for the probability methods, one ``[n, C_i]`` block per segment. Two stand-ins read
the same table: :class:`DeviceSegment` replaces ``SegmentedPlan.subs[i]`` and copies the row-indexed
tensors where a segment plan would have written its results; :class:`StubEvaluator` replaces
``evaluator.sub[i]`` and returns the same arrays as a ``ModelResult``, so
``CompiledPmml.score_matrix_oracle`` (Target stage and label table included) is the reference. The
real segment trees are never walked: what is compared is the aggregation alone.

A segment *yields nothing* where ``V = 0`` (its ``S`` then holds a finite decoy that a reduction
ignoring ``V`` would aggregate) or where ``V = 1`` and ``S`` is NaN; the stub reports both as
``valid = False``, which is what a segment evaluator returns for a row without a prediction.

Exactness: every value is a multiple of 1/4 with magnitude <= 64, every weight a multiple of 1/2
and every probability a multiple of 1/16, so each product and each sum (over at most 256 segments)
is exact in float64 in any order and under FMA contraction; each quotient is then ONE correctly
rounded division on both sides. Scores are compared on their fp32 bit patterns.

Not covered, on purpose:

* +-0.0 is in no grid: ``numpy``'s ``max`` / ``min`` over mixed zeros is not a stable reference.
* Tree segments expose at most 16 classes, so the C = 64 / 65 boundary of the kernel's two
  instantiations is out of reach here; the instantiation switch is driven by K alone.
* Category orders: the loader gives a tree the target's declared ``Value`` order first and then its
  own first-appearance order, so without declared values segments DO get orders that differ from
  the ensemble's (``permuted=True``: ``remap_lists`` is not the identity). A ``-1`` entry arises
  only under ``selectFirst`` for a class the first segment lacks; that is not built here.
* An unstable sort among EQUAL segment values cannot change a weighted median: the chosen index
  may move inside the group of equal values, the chosen value cannot (see ``restate``). With zeros
  of both signs excluded there is no row on which it shows, and none is claimed.
"""

import contextlib
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

from flink_jpmml_amd.bench.synth import segmented_pmml, set_target
from flink_jpmml_amd.models.base import ModelResult
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from tests import _boundary as B

F32 = np.float32
NS = "http://www.dmg.org/PMML-4_4"
REG_METHODS = ("selectFirst", "sum", "average", "weightedAverage", "max", "min", "median", "weightedMedian")
VOTE_METHODS = ("majorityVote", "weightedMajorityVote")
PROB_METHODS = ("average", "weightedAverage", "max", "median")
CLS_METHODS = ("selectFirst",) + VOTE_METHODS + PROB_METHODS
TREATMENTS = (None, "skipSegment", "returnMissing")
CLASSES = ("0", "1", "2")
REAL = [(m, False) for m in REG_METHODS] + [(m, True) for m in CLS_METHODS]  # (method, classification)
DECOY = 37.75  # S where V = 0: finite, a multiple of 1/4, larger than any value of the small grids
# probability rows (sixteenths; -1 = NaN): ties at the top after max / average / median are common
TEMPLATES = np.array([[8, 8, 0], [4, 8, 4], [8, 4, 4], [0, 8, 8], [-1, 8, 8], [16, 0, 0], [6, 6, 4], [4, 4, 8],
                      [8, -1, 8], [2, 6, 8]], dtype=np.float64)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


# --------------------------------------------------------------------------- documents


def leaf_doc(K: int, method: str, weights, classification: bool = False, permuted: bool = False,
             treatment: Optional[str] = None, target: Optional[dict] = None) -> str:
    """K one-leaf tree segments, segment i under ``f<i> greaterThan 0`` with ``weights[i]``.
    Classification leaves carry a ``ScoreDistribution`` over :data:`CLASSES` (so the segment plans
    expose probabilities); ``permuted`` leaves the target's values undeclared and lists the
    classes of segment i rotated by i, which gives the segments different category orders."""
    dd = "".join(f'<DataField name="f{j}" optype="continuous" dataType="float"/>' for j in range(K))
    if classification:
        vals = "" if permuted else "".join(f'<Value value="{c}"/>' for c in CLASSES)
        dd += f'<DataField name="y" optype="categorical" dataType="integer">{vals}</DataField>'
    else:
        dd += '<DataField name="y" optype="continuous" dataType="double"/>'
    ms = '<MiningSchema><MiningField name="y" usageType="target"/>' + "".join(
        f'<MiningField name="f{j}"/>' for j in range(K)) + "</MiningSchema>"
    fn = "classification" if classification else "regression"
    segs = []
    for i in range(K):
        if classification:
            order = [CLASSES[(i + j) % 3] for j in range(3)] if permuted else list(CLASSES)
            dist = "".join(f'<ScoreDistribution value="{c}" recordCount="1"/>' for c in order)
            node = f'<Node id="1" score="{order[0]}"><True/>{dist}</Node>'
        else:
            node = '<Node id="1" score="1"><True/></Node>'
        segs.append(f'<Segment id="{i + 1}" weight="{float(weights[i])!r}"><SimplePredicate field="f{i}" '
                    f'operator="greaterThan" value="0"/><TreeModel functionName="{fn}">{ms}{node}</TreeModel>'
                    '</Segment>')
    mpt = f' missingPredictionTreatment="{treatment}"' if treatment else ""
    txt = (f'<PMML version="4.4" xmlns="{NS}"><DataDictionary>{dd}</DataDictionary><MiningModel '
           f'functionName="{fn}">{ms}<Segmentation multipleModelMethod="{method}"{mpt}>{"".join(segs)}'
           '</Segmentation></MiningModel></PMML>')
    return set_target(txt, **target) if target else txt


def dyadic_weights(txt: str) -> str:
    """The ``weight`` attribute of segment i rewritten to (1 + i % 4) / 2: weighted sums stay exact."""
    import re

    count = [0]

    def w(m):
        k = count[0]
        count[0] += 1
        return f'{m.group(1)}weight="{(1 + k % 4) / 2!r}"'

    return re.sub(r'(<Segment id="\d+" )weight="[^"]+"', w, txt)


@functools.lru_cache(maxsize=None)
def real_doc(method: str, classification: bool, treatment: Optional[str]) -> str:
    """A ``segmented_pmml`` document whose segment trees can yield nothing (``nullPrediction``),
    with integer leaves / class labels and dyadic segment weights."""
    seed = 3 + len(method) + (17 if classification else 0)
    txt = segmented_pmml(method, classification, n_segments=5 + seed % 4, depth=3, n_features=6, n_classes=3,
                         seed=seed, missing_treatment=treatment)
    txt = B.integer_leaves(B.null_prediction(txt), labels=CLASSES if classification else (), modulus=31)
    return dyadic_weights(txt)


def real_inputs(txt: str) -> np.ndarray:
    X = B.boundary_matrix(B.split_cuts(txt, 6), 2049, seed=5)
    X.setflags(write=False)
    return X


# --------------------------------------------------------------------------- a case


class Case:
    def __init__(self, name: str, K: int, method: str, weights, X, S, V, P=None, classification=False,
                 permuted=False, treatment=None, target=None):
        self.name, self.K, self.method, self.weights = name, K, method, np.asarray(weights, dtype=np.float64)
        self.classification, self.permuted, self.treatment, self.target = classification, permuted, treatment, target
        self.X = np.ascontiguousarray(X, dtype=F32)
        self.S = np.ascontiguousarray(S, dtype=F32)
        self.V = np.ascontiguousarray(V, dtype=np.uint8)
        self.P = None if P is None else [np.ascontiguousarray(p, dtype=F32) for p in P]
        self.n = self.X.shape[0]
        assert self.X.shape == (self.n, K) and self.S.shape == (K, self.n) == self.V.shape
        assert not (self.X == 0).any() and (classification or not (self.S == 0).any())  # no zero of either sign
        for a in [self.X, self.S, self.V] + (self.P or []):
            a.setflags(write=False)
        self.probs = classification and method in PROB_METHODS and method != "selectFirst"

    @property
    def txt(self) -> str:
        return leaf_doc(self.K, self.method, self.weights, self.classification, self.permuted, self.treatment,
                        self.target)

    def __repr__(self):
        return self.name


class StubEvaluator:
    """Stands in for ``evaluator.sub[i]``: the case's arrays as that segment's ``ModelResult``."""

    target = None

    def __init__(self, real, case: Case, i: int):
        self.model, self.kind, self.categories = real.model, real.kind, real.categories
        self.case, self.i = case, i

    def evaluate(self, cols) -> ModelResult:
        c, i = self.case, self.i
        assert cols.n == c.n
        s = c.S[i].astype(np.float64)
        valid = c.V[i].astype(bool) & ~np.isnan(s)
        probs = c.P[i].astype(np.float64) if c.P is not None else None
        return ModelResult(self.kind, np.where(valid, s, np.nan), valid, categories=self.categories, probs=probs)

    def compute_outputs(self, cols, res) -> dict:
        return {}


@functools.lru_cache(maxsize=4)
def compiled(txt: str) -> CompiledPmml:
    """The parsed document (the 256-segment ones take seconds): shared by the plan and the oracle."""
    return CompiledPmml.from_string(txt)


@contextlib.contextmanager
def stubbed(case: Case):
    """The case's compiled document while every segment evaluator is replaced by its stub."""
    c = compiled(case.txt)
    ev = c.evaluator
    real = ev.sub
    ev.sub = [StubEvaluator(sub, case, i) for i, sub in enumerate(real)]
    try:
        yield c
    finally:
        ev.sub = real


_REF: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}


def reference(case: Case) -> Tuple[np.ndarray, np.ndarray]:
    """(scores, validity) of the float64 oracle over the stubs — computed once, never changed."""
    if case.name not in _REF:
        with stubbed(case) as c:
            ref, vref = c.score_matrix_oracle(case.X)
        ref.setflags(write=False)
        vref.setflags(write=False)
        _REF[case.name] = (ref, vref)
    return _REF[case.name]


class DeviceSegment:
    """Stands in for ``SegmentedPlan.subs[i]``: copies the case's row-indexed tensors."""

    def __init__(self, case: Case, i: int, device):
        import torch

        self.S = torch.from_numpy(case.S[i].copy()).to(device)
        self.V = torch.from_numpy(case.V[i].copy()).to(device)
        self.P = torch.from_numpy(case.P[i].copy()).to(device) if case.P is not None else None

    def launch(self, X, score, valid, stream=None, probs=None, **kw) -> None:
        assert X.shape[0] == self.S.shape[0]
        score.copy_(self.S)
        valid.copy_(self.V)
        if probs is not None:
            probs.copy_(self.P)


def segmented(plan):
    """The SegmentedPlan of a lowered document (behind its prepare pass, if it has one)."""
    from flink_jpmml_amd.runtime.segmented import SegmentedPlan

    inner = plan if isinstance(plan, SegmentedPlan) else getattr(plan, "inner", None)
    assert isinstance(inner, SegmentedPlan), type(plan)
    return inner


def run_plan(plan, case: Case, device, strided: bool = False, mirrors: bool = False):
    """``plan.launch`` once on the case's whole matrix with the device stand-ins swapped in.
    Returns (score, valid) and, with ``mirrors``, the ``score2`` / ``valid2`` pair as well."""
    import torch

    seg = segmented(plan)
    assert seg.n_subs == case.K
    seg.subs = [DeviceSegment(case, i, device) for i in range(case.K)]
    if strided:
        wide = np.full((case.n, case.K + 3), 97.0, dtype=F32)  # a stride-blind kernel reads TRUE everywhere
        wide[:, : case.K] = case.X
        Xt = torch.from_numpy(wide).to(device)[:, : case.K]
        assert Xt.stride(0) == case.K + 3
    else:
        Xt = torch.from_numpy(case.X.copy()).to(device)
    outs = [torch.full((case.n,), -7.0, dtype=torch.float32, device=device),
            torch.full((case.n,), 9, dtype=torch.uint8, device=device)]
    kw = {}
    if mirrors:
        outs += [torch.full_like(outs[0], -7.0), torch.full_like(outs[1], 9)]
        kw = dict(score2=outs[2], valid2=outs[3])
    plan.launch(Xt, outs[0], outs[1], **kw)
    if device.type == "cuda":
        torch.cuda.synchronize()
    res = [o.cpu().numpy() for o in outs]
    return tuple(r.astype(bool) if r.dtype == np.uint8 else r for r in res)


def assert_same(s, v, ref, vref, what: str) -> None:
    """Validity equal on every row, scores equal on their fp32 bit patterns, NaN where invalid."""
    assert np.array_equal(v, vref), f"{what}: validity differs on rows {np.flatnonzero(v != vref)[:8]}"
    bad = np.flatnonzero(bits(s[vref]) != bits(ref[vref]))
    rows = np.flatnonzero(vref)[bad[:5]]
    assert not len(bad), f"{what}: {len(bad)} of {int(vref.sum())} rows differ, rows {rows}: {s[rows]} != {ref[rows]}"
    assert np.isnan(s[~vref]).all(), f"{what}: a score where the oracle has none"


# --------------------------------------------------------------------------- the grids


def _spell(apply: np.ndarray) -> np.ndarray:
    """[n, K] bool -> X: 1 where the segment applies; FALSE (-1) and UNKNOWN (NaN) alternate."""
    n, K = apply.shape
    r = np.arange(n)[:, None]
    off = np.where((r + r // 6 + np.arange(K)[None, :]) % 2 == 0, F32(-1), F32(np.nan))
    return np.where(apply, F32(1), off).astype(F32)


def _probs_from(idx: np.ndarray) -> np.ndarray:
    """Template indices [n] -> [n, 3] probabilities."""
    t = TEMPLATES[idx]
    return np.where(t < 0, np.nan, t / 16.0)


STATE_W = (0.5, 1.5, 1.0, 1.0)
# all equal / ascending / descending / two equal pairs; x 0.5 (the Target grid) hits exact halves
PATTERNS = np.array([[1, 1, 1, 1], [-1.5, 0.25, 1, 5], [5, 1, 0.25, -1.5], [5, -3, 5, -3]], dtype=np.float64)
CLASS_PATTERNS = np.array([[1, 1, 1, 1], [0, 1, 2, 2], [2, 2, 1, 0], [2, 0, 2, 0]])
TEMPLATE_PATTERNS = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [5, 6, 7, 8], [0, 9, 0, 9]])


@functools.lru_cache(maxsize=None)
def _state_table():
    """K = 4; every segment in one of four states (0 not applying, 1 a value, 2 V = 0, 3 V = 1 and a
    NaN score): all 4**4 combinations x four value patterns, plus one row (1025: a ragged tile)."""
    rows = [(combo, pat) for pat in range(4) for combo in range(256)] + [(0b01010101, 1)]
    n = len(rows)
    state = np.array([[(c >> (2 * i)) & 3 for i in range(4)] for c, _ in rows])  # [n, 4]
    pat = np.array([p for _, p in rows])
    return n, state, pat


def states_case(method: str, classification: bool, treatment: Optional[str] = None, permuted: bool = False,
                target: Optional[dict] = None, tag: str = "states") -> Case:
    n, state, pat = _state_table()
    base = (CLASS_PATTERNS if classification else PATTERNS)[pat].astype(np.float64)  # [n, 4]
    S = np.where(state == 3, np.nan, np.where(state == 2, 2.0 if classification else DECOY, base)).T
    V = (state != 2).T
    P = None
    if classification and method in PROB_METHODS:
        P = []
        for i in range(4):
            p = _probs_from(TEMPLATE_PATTERNS[pat, i])
            p[state[:, i] == 2] = [0.0, 0.0, 1.0]  # decoy where the segment yields nothing
            P.append(p)
    name = "-".join([tag, "cls" if classification else "reg", method, str(treatment)] + (["perm"] if permuted else [])
                    + ([target["id"]] if target else []))
    tg = {k: v for k, v in target.items() if k != "id"} if target else None
    return Case(name, 4, method, STATE_W, _spell(state != 0), S, V, P, classification, permuted, treatment, tg)


VALUE_W = (0.5, 1.5, 1.0, 1.0, 2.0, 2.0)
VALUE_SET = np.array([-64, -7.25, -0.25, 0.25, 0.5, 1.75, 3, 3, 64], dtype=np.float64)


def values_case(method: str) -> Case:
    """K = 6, 513 rows of draws (with repeats) from nine multiples of 1/4 up to +-64; the weights make
    the cumulative weight land exactly on half the total on many rows."""
    rng = np.random.default_rng(11)
    n, K = 513, 6
    S = VALUE_SET[rng.integers(len(VALUE_SET), size=(K, n))]
    apply = rng.random((n, K)) < 0.75
    apply[:64] = True  # rows where all six apply: total weight 8, half of it reached after 0.5 + 1.5 + 2
    V = rng.random((K, n)) < 0.93
    S = np.where(V, S, DECOY)
    return Case(f"values-{method}", K, method, VALUE_W, _spell(apply), S, V, treatment="skipSegment")


CLS_W = (0.5, 0.5, 1.0, 1.0, 2.0)


def classes_case(method: str, permuted: bool) -> Case:
    """K = 5, C = 3, 513 rows: class indices and probability templates drawn at random, so votes
    tie (0.5 + 0.5 against 1.0, one against one) and probabilities tie at the top."""
    rng = np.random.default_rng(13)
    n, K = 513, 5
    S = rng.integers(3, size=(K, n)).astype(np.float64)
    tmpl = rng.integers(len(TEMPLATES), size=(K, n))
    apply = rng.random((n, K)) < 0.7
    V = rng.random((K, n)) < 0.93
    P = [_probs_from(tmpl[i]) for i in range(K)] if method in PROB_METHODS else None
    name = f"classes-{method}" + ("-perm" if permuted else "")
    return Case(name, K, method, CLS_W, _spell(apply), S, V, P, True, permuted, "skipSegment")


TARGETS = [
    dict(id="clip-default", min=-1.0, max=2.0, default=-7.5),
    dict(id="rescale", factor=0.5, constant=0.25),
    dict(id="round", factor=0.5, constant=0.0, cast="round"),
    dict(id="ceiling-clip", min=-2.0, max=4.0, factor=0.5, constant=0.0, cast="ceiling"),
    dict(id="floor-default", factor=0.5, constant=0.25, cast="floor", default=6.0),
]

SIZES = (1, 2, 63, 64, 65, 128, 129, 256)
SIZE_METHODS = (("selectFirst", False), ("median", False), ("weightedMedian", False), ("sum", False),
                ("majorityVote", True), ("max", True))
SIZE_ROWS = 129


def size_case(K: int, method: str, classification: bool) -> Case:
    """129 rows cycling through: only segment 0 applies, only K - 1, only 63, only 64 (clamped to
    K - 1), all, none. The value of segment i names it, so the bit that was read shows."""
    n = SIZE_ROWS
    r = np.arange(n)
    i = np.arange(K)
    only = np.stack([np.zeros(n, int), np.full(n, K - 1), np.full(n, min(63, K - 1)), np.full(n, min(64, K - 1))])
    kind = r % 6
    apply = np.where((kind < 4)[:, None], i[None, :] == only[np.minimum(kind, 3), r][:, None], (kind == 4)[:, None])
    V = (i[:, None] + r[None, :]) % 11 != 3
    if classification:
        S = ((i[:, None] + r[None, :] // 6) % 3).astype(np.float64)
    else:
        S = (i[:, None] % 33 - 16) + 0.25 * (1 + r[None, :] % 3)
    S = np.where(V, S, 2.0 if classification else DECOY)
    P = None
    if classification and method in PROB_METHODS:
        P = [_probs_from((k + r // 6) % len(TEMPLATES)) for k in range(K)]
    w = (1 + i % 4) / 2
    return Case(f"size-K{K}-{method}", K, method, w, _spell(apply), S, V, P, classification, False, "skipSegment")


def inf_case(method: str) -> Case:
    """K = 3: a prescribed +inf / -inf as the chosen or an aggregated value, next to finite rows."""
    inf = np.inf
    S = np.array([[inf, -inf, 1.0, inf, 2.5, -inf, inf, 1.0, -inf],
                  [1.0, 2.0, inf, inf, -inf, -inf, -inf, 2.0, 1.5],
                  [3.0, 3.0, 3.0, 3.0, 3.0, 3.0, -inf, inf, inf]])
    n = S.shape[1]
    apply = np.ones((n, 3), dtype=bool)
    S = np.concatenate([S, S], axis=1)
    apply = np.concatenate([apply, np.tile(np.array([[True, False, True]]), (n, 1))])
    return Case(f"inf-{method}", 3, method, (1.0, 0.5, 0.5), _spell(apply), S, np.ones_like(S, dtype=bool))


@functools.lru_cache(maxsize=None)
def all_cases() -> Tuple[Case, ...]:
    cases: List[Case] = []
    for t in TREATMENTS:
        cases += [states_case(m, False, t) for m in REG_METHODS]
        cases += [states_case(m, True, t) for m in CLS_METHODS]
    cases += [states_case(m, True, "skipSegment", permuted=True) for m in CLS_METHODS]
    cases += [values_case(m) for m in REG_METHODS]
    cases += [classes_case(m, p) for m in CLS_METHODS for p in (False, True)]
    cases += [states_case(m, False, t, target=tg, tag="target") for m in ("selectFirst", "median")
              for tg in TARGETS for t in ((None, "skipSegment") if tg["id"] == "round" else (None,))]
    cases += [size_case(K, m, c) for K in SIZES for m, c in SIZE_METHODS]
    cases += [inf_case(m) for m in REG_METHODS]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def case(name: str) -> Case:
    return {c.name: c for c in all_cases()}[name]


# --------------------------------------------------------------------------- the rules, restated

MUTANTS = ("wmedian-le", "median-lower", "ties-high", "skip-inverted", "select-fallthrough", "round-half-even",
           "unstable-sort")


def _categories(case: Case) -> Tuple[List[str], List[List[int]]]:
    """(ensemble categories, per-segment map of segment class -> ensemble class) as the loader
    orders them: declared values first, else first appearance."""
    seg = [[CLASSES[(i + j) % 3] for j in range(3)] if case.permuted else list(CLASSES) for i in range(case.K)]
    cats = list(seg[0])
    if case.method != "selectFirst":
        for s in seg:
            cats += [c for c in s if c not in cats]
    return cats, [[cats.index(c) if c in cats else -1 for c in s] for s in seg]


def restate(case: Case, mutant: Optional[str] = None):
    """The PMML rules in plain numpy, row by row, with one named deviation switched on by
    ``mutant``. Returns (scores, validity, counters of the edges the rows sit on)."""
    assert mutant is None or mutant in MUTANTS
    K, n, m = case.K, case.n, case.method
    w_all = case.weights
    skip = case.treatment == "skipSegment"
    if mutant == "skip-inverted":
        skip = not skip
    tg = case.target or {}
    cats, remap = _categories(case) if case.classification else (None, None)
    out = np.full(n, np.nan)
    valid = np.zeros(n, dtype=bool)
    stat = dict(nothing=0, half_wmedian=0, even_median=0, top_tie=0, half_round=0)

    def median(v):
        v = np.sort(v)
        lo, hi = v[(len(v) - 1) // 2], v[len(v) // 2]
        if lo != hi:
            stat["even_median"] += 1
        return lo if mutant == "median-lower" else (lo + hi) / 2

    def argmax(acc):
        a = np.where(np.isnan(acc), -1.0, acc)
        top = np.flatnonzero(a == a.max())
        if len(top) > 1:
            stat["top_tie"] += 1
        return top[-1] if mutant == "ties-high" else top[0]

    for r in range(n):
        apply = case.X[r] > 0
        s = case.S[:, r].astype(np.float64)
        okk = case.V[:, r].astype(bool) & ~np.isnan(s)
        use = apply & okk
        anymiss = bool((apply & ~okk).any())
        stat["nothing"] += anymiss
        val, ok = np.nan, False
        if m == "selectFirst":
            pick = use if mutant == "select-fallthrough" else apply
            if pick.any():
                f = int(np.argmax(pick))
                ok = bool(okk[f])
                if ok and case.classification:
                    lab = remap[f][int(s[f])]
                    ok = lab >= 0
                    val = float(cats[lab]) if ok else np.nan
                elif ok:
                    val = s[f]
        elif not case.classification:
            v, w = s[use], w_all[use]
            if len(v):
                if m == "sum":
                    val = v.sum()
                elif m == "average":
                    val = v.sum() / len(v)
                elif m == "weightedAverage":
                    val = (v * w).sum() / w.sum()
                elif m == "max":
                    val = v.max()
                elif m == "min":
                    val = v.min()
                elif m == "median":
                    val = median(v)
                else:
                    # stable ascending order; "unstable-sort" reverses the order among equal values
                    o = np.lexsort((-np.arange(len(v)) if mutant == "unstable-sort" else np.arange(len(v)), v))
                    cw = np.cumsum(w[o])
                    half = 0.5 * cw[-1]
                    stat["half_wmedian"] += bool((cw == half).any())
                    below = int(((cw <= half) if mutant == "wmedian-le" else (cw < half)).sum())
                    val = v[o][min(below, len(v) - 1)]
            ok = len(v) > 0 and (skip or not anymiss) and bool(np.isfinite(val))
        else:
            acc = np.zeros(len(cats))
            if m in VOTE_METHODS:
                for i in np.flatnonzero(use):
                    acc[remap[i][int(s[i])]] += w_all[i] if m == "weightedMajorityVote" else 1.0
            else:
                Pm = np.full((K, len(cats)), np.nan)
                for i in np.flatnonzero(use):
                    Pm[i, remap[i]] = case.P[i][r]
                u = np.flatnonzero(use)
                if len(u):
                    if m == "median":
                        acc = np.array([median(col[~np.isnan(col)]) if (~np.isnan(col)).any() else np.nan
                                        for col in Pm[u].T])
                    elif m == "max":
                        acc = np.maximum(np.nan_to_num(Pm[u]).max(axis=0), 0.0)
                    else:
                        ww = w_all[u] if m == "weightedAverage" else np.ones(len(u))
                        acc = (np.nan_to_num(Pm[u]) * ww[:, None]).sum(axis=0) / ww.sum()
            if use.any():
                val = float(cats[argmax(acc)])
            ok = bool(use.any()) and (skip or not anymiss)
        if not case.classification and tg:
            if tg.get("min") is not None and val < tg["min"]:
                val = tg["min"]
            if tg.get("max") is not None and val > tg["max"]:
                val = tg["max"]
            val = val * tg.get("factor", 1.0) + tg.get("constant", 0.0)
            cast = tg.get("cast")
            if cast == "round":
                if ok and val - np.floor(val) == 0.5:
                    stat["half_round"] += 1
                val = np.round(val) if mutant == "round-half-even" else np.floor(val + 0.5)
            elif cast == "ceiling":
                val = np.ceil(val)
            elif cast == "floor":
                val = np.floor(val)
            if tg.get("default") is not None and not ok:
                val, ok = tg["default"], True
        ok = ok and not np.isnan(val)
        out[r], valid[r] = (val if ok else np.nan), ok
    return out, valid, stat
