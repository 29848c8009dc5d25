"""Named probes of the wide PERFECT tree kernel (csrc/tree_common.h ``wide_tile``), CPU side: the
documents, their inputs, the float64 oracle, what each plan must lower to, the coverage each case
exists for *computed from the plan*, the numpy twin of the kernel (``emulate_wide``) and the named
mutants of a packed plan.

Exactness is the project's own rule (tests/_boundary.py): integer leaves and integer or
power-of-two weights make every sum exact in fp32 in any order, so the oracle and a correct kernel
agree in every bit. Inputs come from ``boundary_matrix`` over the document's own cuts (cut +-2 ulps
and the special values), scored at 1, ROWS - 1, ROWS, ROWS + 1 and 2 ROWS + 33 rows of one matrix,
and once more on a matrix whose first tile has no missing value and whose second tile has one."""

import collections
import functools
import re

import numpy as np
import torch

from tests import _boundary as B

from flink_jpmml_amd.bench.synth import gbdt_pmml, random_forest_pmml
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import (DYN_B, DYN_SLOTS, VAR_NAN_FAST, VAR_NAN_PLANES, TreePlan,
                                           lowering_dry_run)

F32 = np.float32
LO, HI = -100.0, 100.0  # below / above every cut of a synthetic document (standard normal cuts)
MODES = {"sum": 0, "slot": 1, "class": 2, "vote8": 3}


# --------------------------------------------------------------------------- document mutators


def spread_fields(txt: str, F: int) -> str:
    """Every split on its own column, cycling through all ``F`` (both predicates of a split share
    one (field, constant) pair and move together): a small forest then reads every column."""
    seen = {}

    def field(m):
        key = (m.group(1), m.group(3))
        j = seen.setdefault(key, len(seen) % F)
        return f'<SimplePredicate field="f{j}" operator="{m.group(2)}" value="{m.group(3)}"/>'

    return B._PRED.sub(field, txt)


def weighted_vote(txt: str, weights=(0.5, 1, 2, 4)) -> str:
    """``weightedMajorityVote`` with a ``weight`` on every segment (cycling; dyadic: totals exact)."""
    txt = txt.replace('multipleModelMethod="majorityVote"', 'multipleModelMethod="weightedMajorityVote"')
    return re.sub(r'<Segment id="(\d+)">', lambda m: f'<Segment id="{m.group(1)}" weight='
                                                     f'"{weights[(int(m.group(1)) - 1) % len(weights)]}">', txt)


def integer_intercepts(txt: str) -> str:
    """Softmax intercepts 1, 2, 3, 1, ...: non-zero (``acc_init``) and integer (exact logits)."""
    return re.sub(r'intercept="[^"]+" targetCategory="(\d+)"',
                  lambda m: f'intercept="{int(m.group(1)) % 3 + 1}" targetCategory="{m.group(1)}"', txt)


def _level_fields(txt: str) -> str:
    """Depth-2 trees: the root splits on an even column, its children on odd ones (a node's
    predicate tests its parent's field, so the root's children carry the root's column), so an input
    pattern (even columns, odd columns) in {LO, HI}^2 picks the same leaf position in every tree."""
    out = []
    for line in txt.split("\n"):
        m = re.match(r'^( +)<Node (.*?)<SimplePredicate field="f(\d+)"(.*)$', line)
        if m:
            depth = len(m.group(1)) - 6
            assert depth in (0, 1), line
            j = 2 * (int(m.group(3)) // 2) + depth
            line = f'{m.group(1)}<Node {m.group(2)}<SimplePredicate field="f{j}"{m.group(4)}'
        out.append(line)
    return "\n".join(out)


def positional_leaves(txt: str, C: int, first=None) -> str:
    """Leaf k of every tree (document order: LL, LR, RL, RR) votes class ``k % C``; ``first(t)``
    overrides the class of tree t's first leaf (the one the all-LO row reaches)."""
    head, *trees = txt.split("<Segment id=")
    out = [head]
    for t, seg in enumerate(trees):
        k = [0]

        def leaf(m):
            c = k[0] % C if k[0] or first is None else first(t)
            k[0] += 1
            return f'{m.group(1)}score="{c}"'

        out.append("<Segment id=" + re.sub(r'(<Node id="\d+" )score="[^"]+"', leaf, seg))
    return "".join(out)


# --------------------------------------------------------------------------- documents


def _sum_doc(n_trees, depth, F, seed, p_split=1.0, null=False, modulus=B.LEAF_PRIME, spread=False):
    txt = gbdt_pmml(n_trees=n_trees, depth=depth, n_features=F, seed=seed, p_split=p_split)
    if spread:
        txt = spread_fields(txt, F)
    txt = B.integer_leaves(B.mix_mutants(txt), modulus=modulus)
    return B.null_prediction(txt) if null else txt


def _slot_doc(K, depth, F, seed, spread=False):
    txt = gbdt_pmml(n_trees=5, depth=depth, n_features=F, seed=seed, p_split=1.0, objective="multiclass", n_classes=K)
    if spread:
        txt = spread_fields(txt, F)
    return integer_intercepts(B.integer_leaves(B.mix_mutants(txt), modulus=5))


def _class_doc(C, n_trees, depth, F, seed, spread=False, null=False):
    txt = random_forest_pmml(n_trees=n_trees, depth=depth, n_features=F, n_classes=C, seed=seed, p_split=1.0)
    if spread:
        txt = spread_fields(txt, F)
    txt = B.integer_leaves(B.mix_mutants(txt), labels=[str(c) for c in range(C)])
    txt = weighted_vote(txt)  # (a leaf without a class is refused by the binary lowering: nullPrediction poisons)
    return B.null_prediction(txt) if null else txt


def _vote_doc(C, n_trees, depth, F, seed, p_split=1.0, spread=False, null=False):
    txt = random_forest_pmml(n_trees=n_trees, depth=depth, n_features=F, n_classes=C, seed=seed, p_split=p_split)
    if spread:
        txt = spread_fields(txt, F)
    txt = B.integer_leaves(B.mix_mutants(txt), labels=[str(c) for c in range(C)])
    return B.null_prediction(txt) if null else txt


def _split_first(n_trees, chunk, G, lean):
    """Class of the all-LO leaf per tree: class 0 in every tree a thread of group 0 would walk
    were the chunks ``chunk`` trees long (``(t % chunk) % G == 0``) and in ``lean`` of the others,
    class 1 in the rest. Class 0 wins by far; a counter that wraps at 256 hands the row to class 1."""
    others = [t for t in range(n_trees) if (t % chunk) % G]
    zero = {t for t in range(n_trees) if (t % chunk) % G == 0} | set(others[:lean])
    return lambda t: 0 if t in zero else 1


def _unanimous_doc(C, n_trees, seed, first=None):
    txt = random_forest_pmml(n_trees=n_trees, depth=2, n_features=6, n_classes=C, seed=seed, p_split=1.0)
    return B.mix_mutants(positional_leaves(_level_fields(txt), C, first))


FMAP_READ, FMAP_PREP = (7, 60, 123, 200, 250, 299), 150  # columns the trees read; a column only its interval reads


def _fmap_doc():
    """F = 300, six columns read, and column 150 staged for its ``returnInvalid`` interval alone:
    ``prep[col]`` and ``bad[]`` go through ``feat_map``."""
    from tests import _prep_grid as G

    txt = spread_fields(gbdt_pmml(n_trees=5, depth=2, n_features=300, seed=140, p_split=1.0), len(FMAP_READ))
    txt = B._PRED.sub(lambda m: f'<SimplePredicate field="f{FMAP_READ[int(m.group(1)[1:])]}" operator="{m.group(2)}" '
                                f'value="{m.group(3)}"/>', txt)
    txt = B.integer_leaves(B.mix_mutants(txt))
    return G.treat_field(txt, FMAP_PREP, '<Interval closure="closedOpen" leftMargin="-1" rightMargin="1"/>', None, "",
                         "float", "returnInvalid")


# name -> (builder, F, kind); a document is built, parsed and scored by the oracle once
DOCS = {}
for _n in (1, 7, 8, 9, 12, 14, 15, 17, 19, 137):
    DOCS[f"sum{_n}"] = (functools.partial(_sum_doc, _n, 2 if _n != 19 else 3, 8, 30 + _n), 8, "sum")
    DOCS[f"sum{_n}-null"] = (functools.partial(_sum_doc, _n, 2 if _n != 19 else 3, 8, 30 + _n, null=True), 8, "sum")
DOCS["sum137-f64"] = (functools.partial(_sum_doc, 137, 2, 64, 41, spread=True), 64, "sum")
for _f in (5, 6, 7):
    DOCS[f"sum19-f{_f}"] = (functools.partial(_sum_doc, 19, 3, _f, 50 + _f, spread=True), _f, "sum")
DOCS["sum67-f65"] = (functools.partial(_sum_doc, 67, 2, 65, 61, spread=True), 65, "sum")       # 8 G + 3, G = 8
DOCS["sum183-f70"] = (functools.partial(_sum_doc, 183, 2, 70, 62, spread=True), 70, "sum")     # 23 G - 1
DOCS["sum131-f129"] = (functools.partial(_sum_doc, 131, 2, 129, 63, spread=True), 129, "sum")  # 8 G + 3, G = 16
DOCS["sum367-f135"] = (functools.partial(_sum_doc, 367, 2, 135, 64, spread=True), 135, "sum")  # 23 G - 1
DOCS["sum19-f66"] = (functools.partial(_sum_doc, 19, 3, 66, 65, spread=True), 66, "sum")
DOCS["sum137-f66"] = (functools.partial(_sum_doc, 137, 2, 66, 66, spread=True), 66, "sum")
DOCS["fp8-f65"] = (functools.partial(_sum_doc, 67, 2, 65, 67, spread=True, modulus=29), 65, "sum")
for _k in (3, 8):
    DOCS[f"slot{_k}"] = (functools.partial(_slot_doc, _k, 2, 8, 70 + _k), 8, "slot")
    DOCS[f"slot{_k}-f66"] = (functools.partial(_slot_doc, _k, 3, 66, 72 + _k, spread=True), 66, "slot")
    DOCS[f"class{_k}"] = (functools.partial(_class_doc, _k, 19, 3, 8, 80 + _k), 8, "class")
    DOCS[f"class{_k}-f66"] = (functools.partial(_class_doc, _k, 19, 3, 66, 82 + _k, spread=True), 66, "class")
    DOCS[f"class{_k}-f130"] = (functools.partial(_class_doc, _k, 19, 3, 130, 84 + _k, spread=True), 130, "class")
    DOCS[f"class{_k}-null"] = (functools.partial(_class_doc, _k, 19, 3, 8, 86 + _k, null=True), 8, "class")
for _c in (2, 4):
    DOCS[f"vote{_c}-d2"] = (functools.partial(_vote_doc, _c, 19, 2, 8, 90 + _c), 8, "vote")
    DOCS[f"vote{_c}-d5"] = (functools.partial(_vote_doc, _c, 19, 5, 8, 92 + _c, p_split=0.9), 8, "vote")
    DOCS[f"vote{_c}-d1"] = (functools.partial(_vote_doc, _c, 19, 1, 8, 94 + _c), 8, "vote")
    DOCS[f"vote{_c}-f66"] = (functools.partial(_vote_doc, _c, 19, 3, 66, 96 + _c, spread=True), 66, "vote")
DOCS["vote3-null"] = (functools.partial(_vote_doc, 3, 19, 3, 8, 99, null=True), 8, "vote")
DOCS["fmap300"] = (_fmap_doc, 300, "fmap")
DOCS["cap1020"] = (functools.partial(_unanimous_doc, 4, 1020, 100), 6, "unanimous")
DOCS["cap640"] = (functools.partial(_unanimous_doc, 3, 640, 101), 6, "unanimous")
DOCS["cap1000"] = (functools.partial(_unanimous_doc, 4, 1000, 102), 6, "unanimous")
DOCS["cap640-split"] = (functools.partial(_unanimous_doc, 2, 640, 103, first=_split_first(640, 5, 4, 190)), 6,
                        "unanimous")
DOCS["cap900"] = (functools.partial(_unanimous_doc, 4, 900, 104), 6, "unanimous")
P_SPLIT = {1: 1.0, 2: 1.0, 3: 1.0, 4: 0.9, 6: 0.8, 7: 0.7, 8: 0.65, 9: 0.6, 10: 0.55}
for _d in P_SPLIT:
    DOCS[f"sum9-d{_d}"] = (functools.partial(_sum_doc, 9, _d, 8, 110 + _d, p_split=P_SPLIT[_d]), 8, "sum")
    DOCS[f"vote9-d{_d}"] = (functools.partial(_vote_doc, 3, 9, _d, 8, 120 + _d, p_split=P_SPLIT[_d]), 8, "vote")

UNANIMOUS_ROWS = (3, 255, 256, 544)  # row k: pattern k of (even columns, odd columns) -> leaf LL, LR, RL, RR
PATTERNS = ((LO, LO), (LO, HI), (HI, LO), (HI, HI))
Doc = collections.namedtuple("Doc", "name txt compiled F kind")


@functools.lru_cache(maxsize=None)
def doc(name: str) -> Doc:
    build, F, kind = DOCS[name]
    txt = build()
    return Doc(name, txt, CompiledPmml.from_string(txt), F, kind)


def n_rows(rows_wide: int) -> int:
    return 2 * rows_wide + 33


def prefixes(rows_wide: int):
    return (1, rows_wide - 1, rows_wide, rows_wide + 1, n_rows(rows_wide))


def feature_matrix(d: Doc, rows_wide: int) -> np.ndarray:
    """2 ROWS + 33 boundary rows over the document's own cuts; the unanimous forests also carry
    one row per leaf position on which every tree reaches that position."""
    cuts = B.split_cuts(d.txt, d.F)
    if d.kind == "fmap":
        cuts[FMAP_PREP] = [-1.0, 1.0]  # rows inside, on and outside the interval's bounds
    X = B.boundary_matrix(cuts, n_rows(rows_wide), seed=len(d.txt) % 1000)
    if d.kind == "unanimous":
        for r, (even, odd) in zip(UNANIMOUS_ROWS, PATTERNS):
            X[r, 0::2], X[r, 1::2] = even, odd
    return X


def forced_tiles(X: np.ndarray, rows_wide: int, col: int) -> np.ndarray:
    """2 ROWS rows: no missing value in the first tile, exactly one (row ROWS + 5, column ``col``)
    in the second — one launch that walks the main blob and the NaN blob (or the per-node path)."""
    Y = np.array(X[:2 * rows_wide])
    for f in range(Y.shape[1]):
        c = Y[:, f]
        c[np.isnan(c)] = c[~np.isnan(c)][0]
    Y[rows_wide + 5, col] = np.nan
    return Y


@functools.lru_cache(maxsize=None)
def reference(name: str, rows_wide: int):
    """(X, forced X, (scores, validity) of each) — float64 oracle, computed once, read-only."""
    d = doc(name)
    X = feature_matrix(d, rows_wide)
    col = next(f for f, cuts in enumerate(B.split_cuts(d.txt, d.F)) if cuts)
    Y = forced_tiles(X, rows_wide, col)
    out = (X, Y, d.compiled.score_matrix_oracle(X), d.compiled.score_matrix_oracle(Y))
    for a in (X, Y) + out[2] + out[3]:
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------- the case table

WIDE = dict(layout="perfect", variant="wide")
Case = collections.namedtuple("Case", "name doc opts launch mode rows var nan expect")
# expect: coverage facts (see ``coverage``) that the case exists for, as {key: predicate}
CASES = []


def _case(name, docname, mode, rows, var, nan, opts=None, launch=None, **expect):
    """A SUM plan left to itself slices a forest of 64 trees or more over grid.y (``_auto_splits``:
    up to 16 slices of a few trees each, no chunking left), so every SUM case names its split
    count: one, unless partials are what it is about. The other modes never split."""
    if launch is None:
        launch = dict(splits=1) if mode == "sum" else {}
    CASES.append(Case(name, docname, dict(WIDE, **(opts or {})), launch, MODES[mode], rows, var, nan, expect))


# SUM, 256-row tiles: every 8 / 4 / 2 / 1 remainder of the last dynamic batch, slot wrap-around,
# chunk sizes that differ between the blobs; per-node path under nan_mode="off" and nullPrediction
for _n in (1, 7, 8, 9, 12, 14, 15, 17):
    _case(f"sum{_n}", f"sum{_n}", "sum", 256, 1, "planes", chunks=lambda c: c == 1, tail=lambda t, n=_n: t == {n % 8})
    _case(f"sum{_n}-off", f"sum{_n}", "sum", 256, 1, "off", dict(nan_mode="off"), tail=lambda t, n=_n: t == {n % 8})
    _case(f"sum{_n}-null", f"sum{_n}-null", "sum", 256, 1, "off", tail=lambda t, n=_n: t == {n % 8})
_case("sum137-c24", "sum137", "sum", 256, 1, "planes", dict(max_chunk_trees=24), chunks=lambda c: c == 6,
      batches=lambda b: b == 18 and b > DYN_SLOTS, tail=lambda t: t == {0, 1}, last=lambda n: n == 17)
_case("sum137-c24-off", "sum137", "sum", 256, 1, "off", dict(max_chunk_trees=24, nan_mode="off"),
      chunks=lambda c: c == 6, batches=lambda b: b == 18)
_case("sum137-c24-null", "sum137-null", "sum", 256, 1, "off", dict(max_chunk_trees=24), chunks=lambda c: c == 6)
# 64 staged columns: the second plane leaves the NaN blob 5608 bytes a chunk buffer (112 trees, the main blob 128)
_case("sum137-nan-chunks", "sum137-f64", "sum", 256, 1, "planes", differ=lambda d: d, chunks=lambda c: c == 2,
      chunks_nan=lambda c: c == 2)
# SUM, 128- and 64-row tiles: static groups, mt over 1..15 (asserted over the union of these cases)
STATIC_SUM = [("sum67-f65", 128, (0, 13, 37)), ("sum183-f70", 128, (0, 96, 120, 107, 51)),
              ("sum131-f129", 64, (0, 100)), ("sum367-f135", 64, (0, 208))]
for _d, _r, _caps in STATIC_SUM:
    for _c in _caps:
        _case(f"{_d}-c{_c}", _d, "sum", _r, 1, "planes", dict(max_chunk_trees=_c),
              chunks=(lambda c: c == 1) if not _c else (lambda c: c > 1))
_case("sum183-f70-off", "sum183-f70", "sum", 128, 1, "off", dict(max_chunk_trees=96, nan_mode="off"),
      chunks=lambda c: c == 2)
# fp8 leaves at 128 rows: integer leaves -14..14, scale 14 / 448 = 2^-5, so every e4m3 code and the
# epilogue's product are exact and the oracle itself is the reference
_case("fp8-f65", "fp8-f65", "sum", 128, 2, "off", dict(precision="fp8"))
# SUM with launch(splits=4): partials + pmml_tree_reduce
for _d, _r in (("sum19", 256), ("sum137", 256), ("sum19-f66", 128), ("sum137-f66", 128)):
    _case(f"{_d}-splits4", _d, "sum", _r, 1, "planes", launch=dict(splits=4))
_case("sum1-splits4", "sum1", "sum", 256, 1, "planes", launch=dict(splits=4))  # fewer trees than splits
# SLOT: 5 trees per class; runs straddle groups and (max_chunk_trees) chunks; acc_init
for _k in (3, 8):
    _case(f"slot{_k}", f"slot{_k}", "slot", 256, 1, "planes", cross_group=lambda x: x)
    _case(f"slot{_k}-c8", f"slot{_k}", "slot", 256, 1, "planes", dict(max_chunk_trees=8), cross_chunk=lambda x: x)
    _case(f"slot{_k}-f66-c6", f"slot{_k}-f66", "slot", 128, 1, "planes", dict(max_chunk_trees=6),
          cross_chunk=lambda x: x, cross_group=lambda x: x)
    _case(f"slot{_k}-off", f"slot{_k}", "slot", 256, 1, "off", dict(nan_mode="off", max_chunk_trees=8))
# CLASS: weighted votes, a leaf without a class, C = 3 and C = CMAX
for _k in (3, 8):
    _case(f"class{_k}", f"class{_k}", "class", 256, 1, "planes", weights=lambda w: w)
    _case(f"class{_k}-c8", f"class{_k}", "class", 256, 1, "planes", dict(max_chunk_trees=8), chunks=lambda c: c == 3)
    _case(f"class{_k}-f66", f"class{_k}-f66", "class", 128, 1, "planes", weights=lambda w: w)
    _case(f"class{_k}-f130", f"class{_k}-f130", "class", 64, 1, "planes", weights=lambda w: w)
    _case(f"class{_k}-null", f"class{_k}-null", "class", 256, 1, "off", weights=lambda w: w)
# VOTE8: coded (variant 2) and uncoded (variant 1), C = 2 and C = 4 (the top byte)
for _c in (2, 4):
    _case(f"vote{_c}-d2", f"vote{_c}-d2", "vote8", 256, 2, "planes")
    _case(f"vote{_c}-d5", f"vote{_c}-d5", "vote8", 256, 2, "planes")
    _case(f"vote{_c}-d5-c8", f"vote{_c}-d5", "vote8", 256, 2, "planes", dict(max_chunk_trees=8), chunks=lambda c: c == 3)
    _case(f"vote{_c}-d1", f"vote{_c}-d1", "vote8", 256, 1, "planes")
    _case(f"vote{_c}-f66", f"vote{_c}-f66", "vote8", 128, 1, "planes")  # 2 Fs stride 4 > 65536: no class codes
_case("vote3-null", "vote3-null", "vote8", 256, 2, "off")
# VOTE8 counters: at the cap, past the believed cap, and where only MODE_CLASS is safe
_case("cap1020", "cap1020", "vote8", 256, 2, "planes", dict(max_chunk_trees=64), peak=lambda p: p == 255,
      chunks=lambda c: c > 1)
_case("cap640-c5", "cap640", "vote8", 256, 2, "planes", dict(max_chunk_trees=5), peak=lambda p: p <= 255)
_case("cap1000-c7", "cap1000", "vote8", 256, 2, "planes", dict(max_chunk_trees=7), peak=lambda p: p <= 255)
_case("cap640-split-c5", "cap640-split", "vote8", 256, 2, "planes", dict(max_chunk_trees=5), peak=lambda p: p <= 255)
_case("cap900-c3", "cap900", "class", 256, 1, "planes", dict(max_chunk_trees=3))  # 300 a thread: no VOTE8
_case("fmap300", "fmap300", "sum", 256, 1, "planes")
# every per-depth instantiation but tree_d5.hip
for _d in P_SPLIT:
    _case(f"sum9-d{_d}", f"sum9-d{_d}", "sum", 256, 1, "planes", depth=lambda d, D=_d: d == D)
    _case(f"vote9-d{_d}", f"vote9-d{_d}", "vote8", 256, 1 if _d == 1 else 2, "planes", depth=lambda d, D=_d: d == D)
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
STATIC_SUM_CASES = [c.name for c in CASES if c.mode == 0 and c.rows != 256 and c.var == 1 and c.launch == dict(splits=1)]


def dry_plan(case: Case):
    with lowering_dry_run():
        return TreePlan(doc(case.doc).compiled, torch.device("cpu"), **case.opts)


def peak(plan) -> int:
    """The most trees one thread walks, as the kernel groups them, on either blob."""
    G = 1024 // plan.rows_wide
    return max(TreePlan.vote8_peak(plan.n_trees, c, G) for c in (plan.chunk_trees, plan.chunk_trees_nan) if c)


def launch_splits(case: Case, plan) -> int:
    """Tree slices of every launch of the case (each prefix and the forced matrix): what the case
    names, else what the plan picks on its own, which must be one at every row count."""
    if "splits" in case.launch:
        assert plan.mode == 0 and case.launch["splits"] >= 1
        return case.launch["splits"]
    assert plan.mode != 0 and plan.splits == 1
    auto = {plan._auto_splits(n) for n in prefixes(case.rows) + (2 * case.rows,)}
    assert auto == {1}, (case.name, auto)
    return 1


def case_coverage(case: Case, plan) -> dict:
    return coverage(plan, launch_splits(case, plan))


def coverage(plan, splits: int) -> dict:
    """What a launch of ``plan`` walks, from the plan's own numbers (mirrors ``wide_tile``)."""
    G = 1024 // plan.rows_wide
    dyn = plan.mode == 0 and plan.rows_wide == 256
    tps = -(-plan.n_trees // splits)
    spans = [(tb, min(plan.n_trees, tb + tps)) for tb in range(0, plan.n_trees, tps)]

    def chunks(chunk):
        return [(t0, min(chunk, te - t0)) for tb, te in spans for t0 in range(tb, te, chunk)]

    main = chunks(plan.chunk_trees)
    nan = chunks(plan.chunk_trees_nan) if plan.blob_nan is not None else []
    out = dict(chunks=len(main), chunks_nan=len(nan), differ=bool(nan) and plan.chunk_trees != plan.chunk_trees_nan,
               last=main[-1][1], depth=plan.depth, peak=peak(plan),
               weights=plan.tree_w is not None and len(set(plan.tree_w.cpu().tolist())) > 1)
    if dyn:
        out["tail"] = {nt % DYN_B for _, nt in main + nan}
        out["batches"] = sum(-(-nt // DYN_B) for _, nt in main)
    else:
        out["mt"] = {(nt - g + G - 1) // G for _, nt in main + nan for g in range(G)}
    if plan.mode == 1:
        sl = plan.slots.cpu().numpy()
        out["cross_group"] = any(sl[t] == sl[t + 1] for t in range(plan.n_trees - 1))  # neighbours: groups g, g + 1
        out["cross_chunk"] = any(t0 and sl[t0 - 1] == sl[t0] for t0, _ in main + nan)
    return out


def nan_state(plan) -> str:
    if plan.blob_nan is not None:
        assert plan.variant & VAR_NAN_PLANES and plan.variant & VAR_NAN_FAST and plan.chunk_trees_nan >= 1
        return "planes"
    assert not plan.variant & VAR_NAN_PLANES and plan.chunk_trees_nan == 0
    return "fast" if plan.variant & VAR_NAN_FAST else "off"


def assert_lowering(case: Case, plan) -> None:
    """The case lowers as named, and reaches what it exists for."""
    d = doc(case.doc)
    assert plan.layout == "perfect" and plan.P == 1
    assert (plan.variant & 3, plan.mode, plan.rows_wide) == (case.var, case.mode, case.rows), \
        (case.name, plan.variant, plan.mode, plan.rows_wide)
    assert nan_state(plan) == case.nan, case.name
    used = sorted({int(f) for t in plan.spec.trees for f in t.feature if f >= 0})
    if d.kind == "fmap":
        assert used == list(FMAP_READ)
        used = sorted(used + [FMAP_PREP])
    assert plan.n_stage == len(used) and next(r for r, lim in ((256, 64), (128, 128), (64, 256)) if len(used) <= lim) \
        == case.rows
    if used == list(range(d.F)):
        assert plan.feat_map is None
    else:
        assert plan.feat_map.cpu().tolist() == used
    G = 1024 // plan.rows_wide
    for c in (plan.chunk_trees, plan.chunk_trees_nan):
        cap = case.opts.get("max_chunk_trees", 0)
        assert c <= (cap or plan.n_trees)
        if plan.mode == 0 and plan.rows_wide == 256 and c:
            assert c <= DYN_B * DYN_SLOTS and (c % DYN_B == 0 or c >= plan.n_trees or c < DYN_B)  # whole batches
        if plan.mode == 3:
            assert c % G == 0 or c >= plan.n_trees or c < G
    if plan.mode == 3:
        assert peak(plan) <= 255
    if plan.mode == 1:
        assert plan.acc_init is not None and all(b != 0 for b in plan.acc_init.cpu().tolist())
    cov = case_coverage(case, plan)
    for key, holds in case.expect.items():
        assert holds(cov[key]), (case.name, key, cov[key])


# --------------------------------------------------------------------------- the numpy twin


def emulate_wide(plan, X, use_nan_blob, drop_chunk_tail=False):
    """Per-row result of the wide kernel; ``use_nan_blob`` picks the tile path (NaN blob + two
    planes, as for a tile with missing values) — without it missing values take the per-node
    default-right bits (traverse_chunk_g). ``drop_chunk_tail`` (a mutant): the last tree of every
    chunk is not walked."""
    D, n_t, rec = plan.depth, plan.n_trees, plan.rec_words
    NI, NL = (1 << D) - 1, 1 << D
    PS = plan.rows_wide
    G = 1024 // plan.rows_wide
    stage = plan.feat_map.numpy() if plan.feat_map is not None else np.arange(plan.n_features)
    Xs = X[:, stage].astype(np.float32)
    blob = (plan.blob_nan if use_nan_blob else plan.blob).numpy().view(np.uint32).reshape(n_t, rec)
    planes = np.concatenate([Xs, np.where(np.isnan(Xs), np.float32(np.inf), Xs)], axis=1) if use_nan_blob else Xs
    chunk = plan.chunk_trees_nan if use_nan_blob else plan.chunk_trees
    per_node = not use_nan_blob and not (plan.variant & VAR_NAN_FAST)
    n = len(X)
    rows = np.arange(n)
    C = plan.C
    acc = np.zeros((n, max(C, 1)), np.float64)
    votes = np.zeros((G, n, 4), np.int64)
    pz = np.zeros(n, bool)
    slots = plan.slots.numpy() if plan.slots is not None else None
    tree_w = plan.tree_w.numpy() if plan.tree_w is not None else np.ones(n_t, np.float32)
    codes = plan.variant & 3 == 2 and plan.mode == 3  # VOTE8 class codes in the last-level metas (no leaf array)
    leaf8 = plan.variant & 3 == 2 and plan.mode == 0  # e4m3 leaf pairs in the last-level metas
    if leaf8:
        from flink_jpmml_amd.runtime.plans import dequantize_fp8
    for t in range(n_t):
        if drop_chunk_tail and (t % chunk == chunk - 1 or t == n_t - 1):
            continue
        T = blob[t, 0:2 * NI:2].view(np.float32)
        meta = blob[t, 1:2 * NI:2]
        packed = codes or leaf8
        leaves = None if packed else blob[t, 2 * NI:2 * NI + NL]
        drw = blob[t, 2 * NI + (0 if packed else NL):2 * NI + (0 if packed else NL) + (NI + 31) // 32]
        j = np.ones(n, np.int64)
        miss = np.zeros(n, bool)
        for lev in range(D):
            off = meta[j - 1].astype(np.int64) & (0xFFFF if packed and lev == D - 1 else 0xFFFFFFFF)
            assert (off % (PS * 4) == 0).all()
            x = planes[rows, off // (PS * 4)]
            right = x >= T[j - 1]
            if per_node:
                isn = np.isnan(x)
                right |= isn & (((drw[(j - 1) >> 5] >> ((j - 1) & 31)) & 1) == 1)
                miss |= isn
            j = 2 * j + right
        null_tree = (drw[NI >> 5] >> (NI & 31)) & 1
        if packed:
            pm = meta[(j >> 1) - 1]
            byte = (pm >> np.where(j & 1, 24, 16).astype(np.uint32)) & (3 if codes else 0xFF)
            lv = np.uint32(1) << (np.uint32(8) * byte) if codes else dequantize_fp8(byte.astype(np.uint8)).view(np.uint32)
        else:
            lv = leaves[j - NL]
        poison = miss & (null_tree == 1)
        if plan.mode == 0:
            acc[:, 0] += np.where(poison, np.nan, lv.view(np.float32))
        elif plan.mode == 1:
            acc[~poison, slots[t]] += lv.view(np.float32)[~poison]
        elif plan.mode == 2:
            v = lv.view(np.float32)
            pz |= poison | np.isnan(v)
            ok = ~poison & ~np.isnan(v)
            acc[rows[ok], v[ok].astype(int)] += tree_w[t]
        else:
            g = (t % chunk) % G
            for k in range(4):
                votes[g, ~poison, k] += (lv[~poison] >> (8 * k)) & 0xFF
        pz |= poison
    if plan.mode == 3:
        assert votes.max() <= 255  # a thread's packed u8 counter never carries
        acc = votes.sum(axis=0)[:, :C].astype(np.float64)
    if plan.acc_init is not None:
        acc += plan.acc_init.numpy()[None, :]
    tab = np.array([float(x) for x in plan.labels]) if plan.labels is not None else None
    e = plan.epi_args
    if plan.mode == 0 and e["mode"] == 0:
        return np.where(np.isnan(acc[:, 0]), np.nan, e["a"] * acc[:, 0] + e["b"])
    if plan.mode == 0 and e["mode"] == 1:
        p0 = 1.0 / (1.0 + np.exp(-(e["a"] * acc[:, 0] + e["b"])))
        return np.where(np.isnan(acc[:, 0]), np.nan, tab[np.where(p0 >= 0.5, 0, 1)])
    return np.where(pz, np.nan, tab[np.argmax(acc, axis=1)])  # argmax: ties -> lowest class


class Mutated:
    """A plan with some packed tensors replaced (everything else read through)."""

    def __init__(self, plan, **over):
        self._plan, self._over = plan, over

    def __getattr__(self, k):
        over = object.__getattribute__(self, "_over")
        return over[k] if k in over else getattr(object.__getattribute__(self, "_plan"), k)


def _swap_slots(plan):
    sl = plan.slots.clone()
    t = next(t for t in range(plan.n_trees - 1) if sl[t] != sl[t + 1])  # a run boundary
    sl[t], sl[t + 1] = plan.slots[t + 1], plan.slots[t]
    return Mutated(plan, slots=sl)


def _swap_codes(plan):
    """Left and right class code of every last-level node swapped (bits [23:16] <-> [31:24])."""
    D = plan.depth
    NI, NL = (1 << D) - 1, 1 << D
    out = {}
    for k in ("blob", "blob_nan"):
        if getattr(plan, k) is None:
            continue
        b = getattr(plan, k).numpy().view(np.uint32).reshape(plan.n_trees, plan.rec_words).copy()
        m = b[:, 2 * (NL // 2 - 1) + 1:2 * NI:2]
        b[:, 2 * (NL // 2 - 1) + 1:2 * NI:2] = (m & 0xFFFF) | ((m >> 8) & 0x00FF0000) | ((m << 8) & 0xFF000000)
        out[k] = torch.from_numpy(b.reshape(-1).view(np.int32))
    return Mutated(plan, **out)


# name -> (applies to a plan, the mutated plan, emulate_wide options)
PLAN_MUTANTS = {
    "dropped last tree of a chunk": (lambda p: True, lambda p: p, dict(drop_chunk_tail=True)),
    "tree_slot swapped across a run boundary": (lambda p: p.mode == 1, _swap_slots, {}),
    "tree_w rotated by one": (lambda p: p.mode == 2 and p.tree_w is not None,
                              lambda p: Mutated(p, tree_w=torch.roll(p.tree_w, 1)), {}),
    "class code left and right swapped": (lambda p: p.mode == 3 and p.variant & 3 == 2, _swap_codes, {}),
}
