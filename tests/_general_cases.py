"""Deterministic documents for the GENERAL tree layout (the predicate VM of ``tree.hip``:
``gen_eval`` / ``gen_walk`` / ``tree_general_kernel``, packed by ``runtime/general_tree.py``), a
plain float64 reference walker over the builder's own structure, and named mutants of
``pack_general``'s output.

Every node carries an integer score from a running counter (``k % 251 - 125``, as
``_boundary.integer_leaves``): no parent, child or sibling shares it, so the score names the node a
walk ended on, and a regression sum over 16 trees (dyadic weights, a power-of-two weight sum) is
exact in fp32 in any order. Inputs are ``_boundary.boundary_matrix`` cells over the document's own
constants (+-2 ulps, special values); the categorical column holds its codes and NaN only.

The reference walker evaluates predicates on Python floats with PMML's three-valued logic and
tallies what the rows reach: (leaf opcode, negated, outcome), (compound operator, outcome) and
the walk's exit kind. The CPU tests turn those tallies into conditions.

Families: a single regression tree; 16-tree ``average`` / ``sum`` / ``weightedAverage`` ensembles; a
3-class ``majorityVote`` forest; a classification ``average`` forest with integer
``ScoreDistribution`` payloads (exact class means); a scorecard whose ``ComplexPartialScore``
attributes read an integer column per record (the kernel's ``vcol``). Widths: F = 5 (features
staged in LDS) and F = 66 (predicates on columns at and above 64: read lazily from global memory).
The last section holds the boundary inputs for the sibling-mixture walk (``gen_mixture``)."""

import functools
import math
from collections import Counter
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import _boundary as B

F32 = np.float32
NS = "http://www.dmg.org/PMML-4_4"
CATS = "abcde"
ROWS = 2049
N_TREES = 16
STRATEGIES = ["none", "lastPrediction", "nullPrediction", "defaultChild"]
NO_TRUE = ["returnNullPrediction", "returnLastPrediction"]
FAMILIES = ["single", "average", "sum", "weighted", "vote", "dist"]
WIDTHS = [5, 66]
WEIGHTS = [0.5, 0.5, 1.0, 2.0]  # per tree, cycling: 16 trees sum to 16 (a power of two)
TRUE, FALSE = ("true",), ("false",)

# field preparation of the ``prep`` cases (all constants fp32 numbers: the prepared value is the
# same number in float64 and in fp32)
MISSING_REPL, CLAMP, INTERVAL = 0.125, (-0.75, 0.5), (-4.0, 4.0)
INITIAL_SCORE = 7
VCOL_FILLERS = 48  # extra characteristics of the F = 66 scorecard


@dataclass
class Node:
    k: int  # preorder index within its tree (= the packed node index minus the tree's base)
    id: str
    pred: tuple
    depth: int
    score: Optional[int] = None  # regression value or class index; None: no ``score`` attribute
    dist: Optional[Tuple[int, ...]] = None  # integer ScoreDistribution payload per class
    children: List["Node"] = field(default_factory=list)
    default: Optional["Node"] = None
    vcol: bool = False  # scorecard attribute whose points are 2 * (the leaf column) + 3 per record


def S(f, op, v=None):
    return ("simple", f, op, v)


def IN(f, op, vals, kind="string"):
    return ("set", f, op, tuple(vals), kind)


def C(op, *parts):
    return ("compound", op, tuple(parts))


class Builder:
    """One document: ``F`` input columns (F - 1 continuous ``x<j>`` and the categorical ``c``), of
    which predicates read four continuous ones (``q``; at F = 66 columns 64, 3, 63 and 40) and c."""

    def __init__(self, F: int, family: str):
        self.F, self.family = F, family
        self.names = [f"x{j}" for j in range(F - 1)] + ["c"]
        self.q = self.names[:4] if F == 5 else ["x64", "x3", "x63", "x40"]
        self.col = {n: j for j, n in enumerate(self.names)}
        self.serial = 0  # document-wide node counter: scores and ids
        self.ci = 0
        self.cat = self.catalogue()

    # -- predicates
    def catalogue(self) -> List[tuple]:
        a, b, c, d = self.q
        lt, le, gt, ge = "lessThan", "lessOrEqual", "greaterThan", "greaterOrEqual"
        simple = [
            S(a, lt, "0.3"), S(b, le, "0.7"), S(c, gt, "-0.45"), S(d, ge, "0.1"),  # not fp32 numbers
            S(b, lt, "0.5"), S(c, le, "-0.75"), S(d, gt, "0.25"), S(a, ge, "-1.5"),  # fp32 numbers
            S(a, "equal", "0"), S(b, "notEqual", "0"), S(c, "equal", "0.1"), S(d, "notEqual", "0.1"),
            S("c", "equal", "b"), S("c", "notEqual", "d"), S(d, "equal", "0.25"),
            S(a, lt, "1e39"), S(b, le, "1e39"), S(c, gt, "1e39"), S(d, ge, "1e39"),
            S(b, lt, "-1e39"), S(c, le, "-1e39"), S(d, gt, "-1e39"), S(a, ge, "-1e39"),
            S(a, "isMissing"), S(c, "isNotMissing"), S("c", "isMissing"), S(b, "isNotMissing"),
        ]
        sets = [
            IN("c", "isIn", "a"), IN("c", "isNotIn", "bce"), IN("c", "isIn", CATS), IN("c", "isNotIn", "a"),
            IN("c", "isIn", "ace"), IN("c", "isNotIn", CATS),
            IN(b, "isIn", ["123.5", "-77.25"], "real"),  # values no row holds
            IN(a, "isNotIn", ["0.1", "0.3", "-1.5"], "real"),  # only -1.5 is an fp32 number
        ]
        compound = [
            C("and", S(a, lt, "0.3"), S(b, ge, "0.5")),
            C("or", S(c, le, "-0.75"), S(d, gt, "0.25"), S("c", "equal", "b")),
            C("xor", S(a, ge, "-1.5"), S(d, lt, "0.1")),
            C("surrogate", S(b, le, "0.7"), S(c, gt, "-0.45")),
            C("surrogate", S(a, lt, "0.3"), S(d, ge, "0.1"), TRUE),
            C("surrogate", S(c, "equal", "0"), IN("c", "isIn", "ab"), FALSE),
            C("and", S(a, "isNotMissing"), S(b, lt, "1e39"), S(c, gt, "-1e39"), S(d, "notEqual", "0.1")),
            C("or", S(a, "isMissing"), S(b, gt, "0.7")),
            C("xor", S(b, lt, "0.5"), IN("c", "isNotIn", "de"), S(c, ge, "-0.45")),
            C("surrogate", S(d, lt, "0.25"), S(a, le, "0"), S(b, ge, "0"), S(c, lt, "0.1")),  # all may be UNKNOWN
            # three deep, mixed order
            C("and", C("or", S(a, lt, "0.3"), C("xor", S(b, ge, "0.5"), S(c, le, "-0.75"))),
              C("surrogate", S(d, ge, "0.1"), S(a, gt, "-1.5"))),
            C("or", C("and", S(b, le, "0.7"), C("surrogate", S(c, gt, "-0.45"), S(d, lt, "0.25"), TRUE)),
              C("xor", S(a, "equal", "0"), S("c", "notEqual", "d"))),
            C("xor", C("surrogate", C("and", S(a, ge, "-1.5"), S(b, lt, "0.5")), S(c, "isMissing")),
              C("or", S(d, le, "0.1"), IN("c", "isIn", "a"))),
            C("surrogate", C("xor", S(c, lt, "0.1"), C("or", S(d, gt, "0.25"), S(a, le, "0.3"))),
              C("and", S(b, gt, "0"), S("c", "isNotMissing")), FALSE),
        ]
        out = []
        for i in range(max(len(simple), len(sets), len(compound))):  # interleave the three kinds
            out += [lst[i] for lst in (simple, compound, sets) if i < len(lst)]
        return out

    def and32(self) -> tuple:
        """An ``and`` of exactly 32 simple predicates (a full register stack). The first operand (the
        deepest stack entry) and the last one each decide it on their own rows; the 30 between hold
        for every row without an infinity or a missing value in the four columns."""
        a, b, c, d = self.q
        mostly = [S(a, "lessThan", "1e39"), S(b, "greaterThan", "-1e39"), S(c, "isNotMissing"), S(d, "notEqual", "0.1"),
                  S(b, "lessOrEqual", "1e39"), S(c, "greaterOrEqual", "-1e39"), S(d, "lessThan", "1e39"),
                  S(a, "greaterThan", "-1e39"), S(a, "isNotMissing"), S(c, "lessThan", "1e39"), S(b, "notEqual", "0")]
        mid = [mostly[i % len(mostly)] for i in range(30)]
        return C("and", S(a, "lessThan", "0.3"), *mid, S(b, "greaterOrEqual", "0.5"))

    def special_children(self) -> List[tuple]:
        """Children of tree 0's root, which every row with a TRUE root predicate evaluates in turn."""
        a, b, c, d = self.q
        return [self.and32(),
                C("surrogate", S(d, "lessThan", "0.25"), S(b, "greaterOrEqual", "0"), S(c, "lessThan", "0.1"),
                  S("c", "equal", "b")),  # UNKNOWN on the rows that hold the first column only
                C("xor", S(b, "lessThan", "0.5"), IN("c", "isNotIn", "de"), S(d, "isMissing")),
                IN("c", "isIn", "ace"),
                S(d, "greaterOrEqual", "0.1")]

    def next_pred(self) -> tuple:
        p = self.cat[self.ci % len(self.cat)]
        self.ci += 1
        return p

    # -- trees
    def tree(self, t: int, depth: int) -> Node:
        self.k = 0
        a = self.q[0]
        root_pred = S(a, "greaterThan", "-1e39") if t == 0 else TRUE  # FALSE at -inf, UNKNOWN when missing
        return self.node(root_pred, 0, depth, special=t == 0, root_score=t % 4 != 1)

    def node(self, pred, d, depth, special=False, root_score=True) -> Node:
        k, s = self.k, self.serial
        self.k += 1
        self.serial += 1
        nd = Node(k, f"n{s}", pred, d)
        if self.family in ("vote", "dist"):
            nd.score = s % 3
            if self.family == "dist":
                nd.dist = tuple((s * (c + 2) + c) % 7 for c in range(3))
                nd.score = int(np.argmax(nd.dist))
        else:
            nd.score = s % B.LEAF_PRIME - B.LEAF_PRIME // 2
        if d == depth or (d >= 1 and s % 5 == 3):
            return nd
        if special:
            preds = self.special_children()
        else:
            nc = 2 + s % 4
            preds = [self.next_pred() for _ in range(nc - 1)] + [TRUE if s % 3 == 0 else self.next_pred()]
        nd.children = [self.node(p, d + 1, depth) for p in preds]
        if special:
            nd.default = nd.children[1]
        else:
            if s % 4 != 1:
                nd.default = nd.children[s % len(preds)]
            if (d > 0 and s % 4 == 2) or (d == 0 and not root_score):
                nd.score = None
        near = [n.score for n in nd.children + [nd] if n.score is not None]
        if self.family not in ("vote", "dist"):
            assert len(set(near)) == len(near), "parent, child or sibling scores collide"
        return nd

    def characteristic(self, t: int) -> Node:
        """Scorecard characteristic ``t`` as the tree it lowers to: a root without score whose
        children are the attributes (first TRUE one wins); one of them scores the leaf column."""
        self.k = 1
        self.serial += 1
        root = Node(0, f"ch{t}", TRUE, 0)
        if t == 0:
            preds = self.special_children()
        else:
            nc = 2 + t % 4
            preds = [self.next_pred() for _ in range(nc - 1)] + [TRUE if t % 3 == 0 else self.next_pred()]
        for j, p in enumerate(preds):
            root.children.append(Node(self.k, f"ch{t}a{j}", p, 1, score=self.serial % B.LEAF_PRIME - B.LEAF_PRIME // 2,
                                      vcol=j == t % len(preds)))
            self.k += 1
            self.serial += 1
        return root

    def filler(self, t: int, name: str) -> Node:
        """A two-attribute characteristic on a column nothing else reads: with enough of them the
        derive pass hands the tree kernel more than 64 columns (features stay in global memory)."""
        root = Node(0, f"ch{t}", TRUE, 0)
        for j, p in enumerate((S(name, "greaterOrEqual", "0"), TRUE)):
            root.children.append(Node(j + 1, f"ch{t}a{j}", p, 1, score=self.serial % B.LEAF_PRIME - B.LEAF_PRIME // 2))
            self.serial += 1
        return root

    def scorecard(self, chars: List[Node]) -> str:
        dd = "".join(f'<DataField name="{n}" optype="continuous" dataType="double"/>' for n in self.names[:-1])
        dd += '<DataField name="c" optype="categorical" dataType="string">' + "".join(
            f'<Value value="{v}"/>' for v in CATS) + "</DataField>"
        dd += '<DataField name="y" optype="continuous" dataType="double"/>'
        ms = '<MiningSchema><MiningField name="y" usageType="target"/>' + "".join(
            f'<MiningField name="{n}"/>' for n in self.names) + "</MiningSchema>"
        cps = (f'<ComplexPartialScore><Apply function="+"><Apply function="*"><FieldRef field="{self.q[3]}"/>'
               '<Constant>2</Constant></Apply><Constant>3</Constant></Apply></ComplexPartialScore>')
        body = ""
        for ch in chars:
            body += f'<Characteristic name="{ch.id}">' + "".join(
                f'<Attribute partialScore="{a.score}">{self.pred_xml(a.pred)}{cps if a.vcol else ""}</Attribute>'
                for a in ch.children) + "</Characteristic>"
        return (f'<PMML version="4.4" xmlns="{NS}"><DataDictionary>{dd}</DataDictionary><Scorecard '
                f'functionName="regression" initialScore="{INITIAL_SCORE}" useReasonCodes="false">{ms}<Characteristics>'
                f'{body}</Characteristics></Scorecard></PMML>')

    # -- XML
    def pred_xml(self, p) -> str:
        if p[0] == "true":
            return "<True/>"
        if p[0] == "false":
            return "<False/>"
        if p[0] == "simple":
            v = f' value="{p[3]}"' if p[3] is not None else ""
            return f'<SimplePredicate field="{p[1]}" operator="{p[2]}"{v}/>'
        if p[0] == "set":
            return (f'<SimpleSetPredicate field="{p[1]}" booleanOperator="{p[2]}"><Array type="{p[4]}" n="{len(p[3])}">'
                    + " ".join(p[3]) + "</Array></SimpleSetPredicate>")
        return f'<CompoundPredicate booleanOperator="{p[1]}">' + "".join(self.pred_xml(q) for q in p[2]) + \
            "</CompoundPredicate>"

    def node_xml(self, nd: Node) -> str:
        score = f' score="{nd.score}"' if nd.score is not None else ""
        dflt = f' defaultChild="{nd.default.id}"' if nd.default is not None else ""
        dist = ""
        if nd.dist is not None:
            dist = "".join(f'<ScoreDistribution value="{c}" recordCount="1" probability="{p}"/>'
                           for c, p in enumerate(nd.dist))
        return (f'<Node id="{nd.id}"{score}{dflt}>{self.pred_xml(nd.pred)}{dist}'
                + "".join(self.node_xml(c) for c in nd.children) + "</Node>")

    def document(self, trees: List[Node], strategy: str, no_true: str, prep: bool) -> str:
        a, _, c, d = self.q
        dd = ""
        for n in self.names[:-1]:
            kids = f'<Interval closure="closedClosed" leftMargin="{INTERVAL[0]}" rightMargin="{INTERVAL[1]}"/>' \
                if prep and n == d else ""
            dd += f'<DataField name="{n}" optype="continuous" dataType="double">{kids}</DataField>'
        dd += '<DataField name="c" optype="categorical" dataType="string">' + "".join(
            f'<Value value="{v}"/>' for v in CATS) + "</DataField>"
        cls = self.family in ("vote", "dist")
        if cls:
            dd += '<DataField name="y" optype="categorical" dataType="string"><Value value="0"/><Value value="1"/>' \
                  '<Value value="2"/></DataField>'
        else:
            dd += '<DataField name="y" optype="continuous" dataType="double"/>'
        treat = {}
        if prep:
            treat = {a: f' missingValueReplacement="{MISSING_REPL}"',
                     c: f' outliers="asExtremeValues" lowValue="{CLAMP[0]}" highValue="{CLAMP[1]}"',
                     d: ' invalidValueTreatment="returnInvalid"'}
        ms = '<MiningSchema><MiningField name="y" usageType="target"/>' + "".join(
            f'<MiningField name="{n}"{treat.get(n, "")}/>' for n in self.names) + "</MiningSchema>"
        ms_in = '<MiningSchema><MiningField name="y" usageType="target"/>' + "".join(
            f'<MiningField name="{n}"/>' for n in self.names) + "</MiningSchema>"
        fn = "classification" if cls else "regression"

        def tree(root, schema):
            return (f'<TreeModel functionName="{fn}" missingValueStrategy="{strategy}" '
                    f'noTrueChildStrategy="{no_true}">{schema}{self.node_xml(root)}</TreeModel>')

        if self.family == "single":
            model = tree(trees[0], ms)
        else:
            method = {"average": "average", "sum": "sum", "weighted": "weightedAverage", "vote": "majorityVote",
                      "dist": "average"}[self.family]
            segs = "".join(f'<Segment id="{i}" weight="{WEIGHTS[i % 4]}"><True/>{tree(r, ms_in)}</Segment>'
                           for i, r in enumerate(trees))
            model = (f'<MiningModel functionName="{fn}">{ms}<Segmentation multipleModelMethod="{method}">{segs}'
                     "</Segmentation></MiningModel>")
        return f'<PMML version="4.4" xmlns="{NS}"><DataDictionary>{dd}</DataDictionary>{model}</PMML>'

    # -- inputs
    def cuts(self, trees: List[Node], prep: bool) -> List[List[float]]:
        cuts: List[set] = [set() for _ in self.names]

        def visit(p):
            if p[0] == "simple" and p[3] is not None and p[1] != "c":
                cuts[self.col[p[1]]].add(float(p[3]))
            elif p[0] == "set" and p[4] == "real":
                cuts[self.col[p[1]]].update(float(v) for v in p[3])
            elif p[0] == "compound":
                for q in p[2]:
                    visit(q)

        def walk(nd):
            visit(nd.pred)
            for c in nd.children:
                walk(c)

        for r in trees:
            walk(r)
        if prep:
            cuts[self.col[self.q[2]]].update(CLAMP)
            cuts[self.col[self.q[3]]].update(INTERVAL)
        return [sorted(max(-B.FLT_MAX, min(B.FLT_MAX, v)) for v in s) for s in cuts]  # +-inf: a special value

    def inputs(self, trees: List[Node], prep: bool, seed: int) -> np.ndarray:
        with np.errstate(over="ignore"):  # FLT_MAX + 1 ulp is +inf
            X = np.array(B.boundary_matrix(self.cuts(trees, prep), ROWS, seed))
        codes = (np.arange(ROWS) * 5 + 3) % (len(CATS) + 1)
        col = np.where(codes == len(CATS), np.nan, codes).astype(F32)
        X[:, -1] = col[np.random.default_rng(seed + 1).permutation(ROWS)]
        if self.family == "vcol":  # the leaf column holds small integers (and NaN): sums stay exact
            k = np.arange(ROWS)
            col = np.where(k % 16 == 5, np.nan, (k * 7) % 17 - 8).astype(F32)
            X[:, self.col[self.q[3]]] = col[np.random.default_rng(seed + 2).permutation(ROWS)]
        X[0] = X[1] = X[3] = X[4] = np.nan
        X[2] = 0.0
        X[3, self.col[self.q[0]]], X[4, self.col[self.q[0]]] = 0.0, -1.5  # all missing but the root's column
        return X


# --------------------------------------------------------------------------- the reference walker

T_, F_, U_ = "T", "F", "U"
LEAF_OP = {"lessThan": ("GE", 1), "lessOrEqual": ("GE", 1), "greaterThan": ("GE", 0), "greaterOrEqual": ("GE", 0),
           "equal": ("EQ", 0), "notEqual": ("EQ", 1), "isMissing": ("ISMISS", 0), "isNotMissing": ("NOTMISS", 0),
           "isIn": ("SET", 0), "isNotIn": ("SET", 1)}
# what every case's rows must reach
LEAF_OUTCOMES = [(op, n, o) for op in ("GE", "EQ", "SET") for n in (0, 1) for o in (T_, F_, U_)] + [
    (op, 0, o) for op in ("ISMISS", "NOTMISS") for o in (T_, F_)] + [("TRUE", 0, T_), ("FALSE", 0, F_)]
COMPOUND_OUTCOMES = [(op, o) for op in ("and", "or", "xor", "surrogate") for o in (T_, F_, U_)]


def allowed_exits(strategy: str, no_true: str, family: str = "") -> List[str]:
    if family == "vcol":  # scorecards: the root is always TRUE and never scores
        return ["leaf", "no_true_null", "leaf_column_missing"]
    out = ["leaf", "root_not_true", "no_true_last" if no_true == "returnLastPrediction" else "no_true_null"]
    out += {"none": [], "lastPrediction": ["last_on_unknown"], "nullPrediction": ["null_on_unknown"],
            "defaultChild": ["default_taken", "default_absent"]}[strategy]
    if strategy == "lastPrediction" or no_true == "returnLastPrediction":
        out.append("no_score")
    return out


class Walker:
    """PMML TreeModel scoring of one row at a time, on Python floats."""

    def __init__(self, strategy: str, no_true: str):
        self.strategy, self.no_true = strategy, no_true
        self.leaf, self.compound, self.exits = Counter(), Counter(), Counter()
        self.and32 = Counter()
        self.hits = Counter()  # (tree, node k) -> rows scored by it
        self.vfield = None  # the scorecards' leaf column

    def value(self, f: str, v: str) -> float:
        return float(CATS.index(v)) if f == "c" else float(v)

    def ev(self, p, row: Dict[str, float]) -> str:
        kind = p[0]
        if kind == "true":
            self.leaf["TRUE", 0, T_] += 1
            return T_
        if kind == "false":
            self.leaf["FALSE", 0, F_] += 1
            return F_
        if kind == "compound":
            vals = [self.ev(q, row) for q in p[2]]  # every operand is evaluated (as the VM does)
            op = p[1]
            if op == "and":
                r = F_ if F_ in vals else (U_ if U_ in vals else T_)
            elif op == "or":
                r = T_ if T_ in vals else (U_ if U_ in vals else F_)
            elif op == "xor":
                r = U_ if U_ in vals else (T_ if vals.count(T_) % 2 else F_)
            else:  # surrogate: the first operand that is not UNKNOWN
                r = next((v for v in vals if v != U_), U_)
            self.compound[op, r] += 1
            if len(vals) == 32:
                rest_true = all(v == T_ for v in vals[1:-1])
                if rest_true and vals[0] == F_ and vals[-1] == T_:
                    self.and32["first_decides"] += 1
                if rest_true and vals[0] == T_ and vals[-1] == F_:
                    self.and32["last_decides"] += 1
                if r == T_:
                    self.and32["true"] += 1
            return r
        x = row[p[1]]
        miss = math.isnan(x)
        opcode, neg = LEAF_OP[p[2]]
        if kind == "simple":
            op = p[2]
            if op == "isMissing":
                r = T_ if miss else F_
            elif op == "isNotMissing":
                r = F_ if miss else T_
            elif miss:
                r = U_
            else:
                v = self.value(p[1], p[3])
                r = T_ if {"lessThan": x < v, "lessOrEqual": x <= v, "greaterThan": x > v, "greaterOrEqual": x >= v,
                           "equal": x == v, "notEqual": x != v}[op] else F_
        else:
            if miss:
                r = U_
            else:
                inside = any(x == self.value(p[1], v) for v in p[3])
                r = T_ if inside == (p[2] == "isIn") else F_
        self.leaf[opcode, neg, r] += 1
        return r

    def walk(self, root: Node, row: Dict[str, float]) -> Tuple[Optional[Node], str]:
        """``(scoring node or None, exit kind)``."""
        if self.ev(root.pred, row) != T_:
            return None, "root_not_true"
        node = root
        while True:
            if not node.children:
                return node, "leaf"
            nxt = None
            for ch in node.children:
                v = self.ev(ch.pred, row)
                if v == U_ and self.strategy != "none":
                    if self.strategy == "lastPrediction":
                        return node, "last_on_unknown"
                    if self.strategy == "nullPrediction":
                        return None, "null_on_unknown"
                    if node.default is None:
                        return None, "default_absent"
                    self.exits["default_taken"] += 1  # an event, not an exit: the walk goes on
                    nxt = node.default
                    break
                if v == T_:
                    nxt = ch
                    break
            if nxt is None:
                if self.no_true == "returnLastPrediction":
                    return node, "no_true_last"
                return None, "no_true_null"
            node = nxt

    def score_tree(self, t: int, root: Node, row) -> Optional[Node]:
        node, kind = self.walk(root, row)
        if node is not None and node.score is None:
            node, kind = None, "no_score"
        if node is not None and node.vcol and math.isnan(row[self.vfield]):
            node, kind = None, "leaf_column_missing"
        self.exits[kind] += 1
        if node is not None:
            self.hits[t, node.k] += 1
        return node


def prepare_row(b: Builder, x: np.ndarray, prep: bool) -> Tuple[Dict[str, float], bool]:
    row = {n: float(v) for n, v in zip(b.names, x)}
    ok = True
    if prep:
        q0, _, q2, q3 = b.q
        if math.isnan(row[q0]):
            row[q0] = MISSING_REPL
        if not math.isnan(row[q2]):
            row[q2] = min(max(row[q2], CLAMP[0]), CLAMP[1])
        if not math.isnan(row[q3]) and not (INTERVAL[0] <= row[q3] <= INTERVAL[1]):
            ok = False
    return row, ok


@dataclass
class Case:
    family: str
    F: int
    strategy: str
    no_true: str
    prep: bool
    builder: Builder
    trees: List[Node]
    doc: str
    X: np.ndarray
    # the reference walker's result
    score: np.ndarray  # float64 [rows]: value or class index (NaN where invalid)
    valid: np.ndarray
    probs: Optional[np.ndarray]  # dist family: class means
    nodes: np.ndarray  # [rows, trees] preorder index of the scoring node (-1: none)
    walker: Walker

    @property
    def name(self) -> str:
        return f"{self.family}-f{self.F}-{self.strategy}-{self.no_true}" + ("-prep" if self.prep else "")

    @functools.cached_property
    def compiled(self):
        from flink_jpmml_amd.runtime.compiled import CompiledPmml

        return CompiledPmml.from_string(self.doc)

    @functools.cached_property
    def oracle(self):
        """``(score, valid, probs or None)`` of the float64 oracle; guards that fp32 holds them exactly."""
        from tests import _epilogue_cases as E

        s, v, p = E.oracle(self.compiled, self.X)
        if self.family == "dist":
            sums = p[v] * N_TREES
            assert np.array_equal(sums, np.round(sums)) and sums.max() < 2 ** 7  # integer sums: exact class means
        elif self.family != "vote":
            B.assert_fp32_exact(s, v)
        for a in (s, v) + ((p,) if p is not None else ()):
            a.setflags(write=False)
        return s, v, p

    @functools.cached_property
    def packed(self):
        from flink_jpmml_amd.runtime.general_tree import pack_general
        from flink_jpmml_amd.runtime.plans import TreePlan

        c = self.compiled
        if self.family == "vcol":  # the derive pass's view: inputs, then the leaf-column expressions
            from flink_jpmml_amd.runtime.derive import FieldView, plan_field_layout
            from flink_jpmml_amd.runtime.general_tree import lower_general_tree
            from flink_jpmml_amd.runtime.plans import ensemble_spec

            layout = plan_field_layout(c, allow_alias=True)
            assert layout.program is not None
            spec = ensemble_spec(FieldView(c, layout, prepared=True), lower=lower_general_tree)
            self.layout = layout
        else:
            spec = TreePlan._general_spec(c)
        return spec, pack_general(spec.trees, spec.weights, spec.P, c.schema)

    def emulate(self, packed=None, rows=slice(None)):
        """``(score, valid, accumulators)`` of the kernel's numpy twin on the prepared rows."""
        from flink_jpmml_amd.runtime.general_tree import emulate_general
        from test_lowering import _scores

        spec, own = self.packed
        P, ok = self.compiled.prepare(self.X[rows].astype(np.float64))
        if self.family == "vcol":
            child = self.compiled.columns(P).child(self.compiled.evaluator.model.local_transformations)
            P = np.stack([child.get(name) for name in self.layout.columns], axis=1)
        acc = emulate_general(packed or own, P.astype(F32), spec.P, len(spec.trees))
        out = _scores(spec, acc)
        valid = np.isfinite(out) & ok
        return np.where(valid, out, np.nan), valid, acc * spec.epi.get("a", 1.0)


@functools.lru_cache(maxsize=None)
def case(family: str, F: int, strategy: str, no_true: str, prep: bool = False) -> Case:
    b = Builder(F, family)
    n_trees, depth = (1, 3) if family == "single" else (N_TREES, 2)
    if family == "vcol":
        assert (strategy, no_true, prep) == ("none", "returnNullPrediction", False)  # what a scorecard lowers to
        trees = [b.characteristic(t) for t in range(n_trees)]
        if F > 64:
            spare = [n for n in b.names[:-1] if n not in b.q][:VCOL_FILLERS]
            trees += [b.filler(n_trees + i, n) for i, n in enumerate(spare)]
            n_trees = len(trees)
        doc = b.scorecard(trees)
    else:
        trees = [b.tree(t, depth) for t in range(n_trees)]
        doc = b.document(trees, strategy, no_true, prep)
    X = b.inputs(trees, prep, seed=F + len(family))
    w = Walker(strategy, no_true)
    w.vfield = b.q[3]
    score = np.full(ROWS, np.nan)
    valid = np.zeros(ROWS, dtype=bool)
    probs = np.full((ROWS, 3), np.nan) if family == "dist" else None
    nodes = np.full((ROWS, n_trees), -1)
    weights = [WEIGHTS[i % 4] for i in range(n_trees)]
    for r in range(ROWS):
        row, ok = prepare_row(b, X[r], prep)
        got = [w.score_tree(t, root, row) for t, root in enumerate(trees)]
        nodes[r] = [-1 if g is None else g.k for g in got]
        if not ok or any(g is None for g in got):
            continue
        valid[r] = True
        if family == "single":
            score[r] = got[0].score
        elif family == "sum":
            score[r] = sum(g.score for g in got)
        elif family == "vcol":
            score[r] = INITIAL_SCORE + sum(2 * row[w.vfield] + 3 if g.vcol else g.score for g in got)
        elif family == "average":
            score[r] = sum(g.score for g in got) / n_trees
        elif family == "weighted":
            score[r] = sum(wt * g.score for wt, g in zip(weights, got)) / sum(weights)
        elif family == "vote":
            votes = [sum(1 for g in got if g.score == c) for c in range(3)]
            score[r] = votes.index(max(votes))
        else:
            probs[r] = [sum(g.dist[c] for g in got) / n_trees for c in range(3)]
            score[r] = int(np.argmax(probs[r]))
    for a in (X, score, valid, nodes) + ((probs,) if probs is not None else ()):
        a.setflags(write=False)
    return Case(family, F, strategy, no_true, prep, b, trees, doc, X, score, valid, probs, nodes, w)


PAIRS = [(s, n) for s in STRATEGIES for n in NO_TRUE]
CASES = [(f, F, s, n, False) for f in FAMILIES for F in WIDTHS for s, n in PAIRS]
# one case per width with field preparation on fields the predicates read
PREP_CASES = [("sum", 5, "defaultChild", "returnLastPrediction", True),
              ("single", 66, "lastPrediction", "returnNullPrediction", True)]
# the per-record leaf column: a scorecard with ComplexPartialScore attributes (always strategy none)
VCOL_CASES = [("vcol", F, "none", "returnNullPrediction", False) for F in WIDTHS]
ALL_CASES = CASES + PREP_CASES + VCOL_CASES
# one strided launch per width
STRIDED = [("sum", 5, "defaultChild", "returnNullPrediction", False),
           ("average", 66, "nullPrediction", "returnLastPrediction", False)]


def case_id(key) -> str:
    f, F, s, n, prep = key
    return f"{f}-f{F}-{s}-{n}" + ("-prep" if prep else "")


# --------------------------------------------------------------------------- mutants of the packed tables

P_GE, P_SET, P_OR, P_XOR, P_SURR = 3, 7, 9, 10, 11  # runtime/general_tree.py


def _copy(packed: dict) -> dict:
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in packed.items()}


def _first(packed: dict, op: int) -> int:
    """The first instruction with this opcode: for ``P_GE`` the root predicate of tree 0."""
    for i, row in enumerate(packed["preds"]):
        if int(row[0]) & 0xFF == op:
            return i
    raise AssertionError(f"no predicate with opcode {op}")


def _root_child(g: dict, j: int, op: int) -> int:
    """The last instruction (a compound's operator, or the one leaf) of the predicate of child j of
    tree 0's root -- the children every row with a TRUE root predicate evaluates in turn."""
    i = int(g["nodes"][int(g["children"][int(g["nodes"][0, 0]) + j]), 2])
    while int(g["preds"][i + 1, 0]) & 0xFF != 0:
        i += 1
    assert int(g["preds"][i, 0]) & 0xFF == op
    return i


def _opcode(op_from: int, op_to: int, child: int):
    def mutate(cs: Case, g: dict) -> dict:
        i = _root_child(g, child, op_from)
        g["preds"][i, 0] = (int(g["preds"][i, 0]) & ~0xFF) | op_to
        return g
    return mutate


def _negate(cs: Case, g: dict) -> dict:
    g["preds"][_first(g, P_GE), 0] ^= 1 << 8
    return g


def _swap_children(cs: Case, g: dict) -> dict:
    off = int(g["nodes"][0, 0])
    g["children"][[off, off + 1]] = g["children"][[off + 1, off]]
    return g


def _clear_has_score(cs: Case, g: dict) -> dict:
    (t, k), _ = cs.walker.hits.most_common(1)[0]  # the node that scores the most rows
    g["nodes"][int(g["trees"][t, 0]) + k, 1] &= ~(1 << 16)
    return g


def _strategy(cs: Case, g: dict) -> dict:
    g["trees"][0, 1] = (int(g["trees"][0, 1]) & ~7) | ((int(g["trees"][0, 1]) & 7) % 3 + 1)
    return g


def _return_last(cs: Case, g: dict) -> dict:
    g["trees"][:, 1] ^= 1 << 3
    return g


def _shorten_set(cs: Case, g: dict) -> dict:
    g["preds"][_root_child(g, 3, P_SET), 3] -= 1
    return g


def _threshold_ulp(cs: Case, g: dict) -> dict:
    i = _first(g, P_GE)
    t = g["preds"][i, 3:4].copy().view(F32)
    g["preds"][i, 3] = B.ulp_step(t, 1).view(np.int32)[0]
    return g


def _default_sibling(cs: Case, g: dict) -> dict:
    off = int(g["nodes"][0, 0])
    assert int(g["nodes"][0, 3]) == int(g["children"][off + 1])
    g["nodes"][0, 3] = g["children"][off + 2]
    return g


def _max_steps(cs: Case, g: dict) -> dict:
    # pack_general keeps one step of slack (depth + 2 where the deepest walk visits depth + 1
    # nodes; tests/golden/tree_plan_pins.json records that value), so "one less" is counted from
    # what the deepest walk needs
    depth = max(nd_depth(r) for r in cs.trees)
    assert g["max_steps"] == depth + 2
    g["max_steps"] = depth
    return g


def nd_depth(nd: Node) -> int:
    return max([nd.depth] + [nd_depth(c) for c in nd.children])


_SINGLE = ("single", 5, "lastPrediction", "returnNullPrediction", False)
# name -> (the case it belongs to, the change)
MUTANTS = {
    "negate-bit": (_SINGLE, _negate),
    "surrogate-as-or": (_SINGLE, _opcode(P_SURR, P_OR, 1)),
    "xor-as-or": (_SINGLE, _opcode(P_XOR, P_OR, 2)),
    "swap-children": (_SINGLE, _swap_children),
    "clear-has-score": (("sum", 5, "none", "returnNullPrediction", False), _clear_has_score),
    "strategy-bits": (("single", 66, "nullPrediction", "returnNullPrediction", False), _strategy),
    "return-last-bit": (("average", 5, "none", "returnLastPrediction", False), _return_last),
    "shorten-set": (_SINGLE, _shorten_set),
    "threshold-ulp": (("single", 66, "none", "returnNullPrediction", False), _threshold_ulp),
    "default-child-sibling": (("single", 5, "defaultChild", "returnNullPrediction", False), _default_sibling),
    "max-steps": (("single", 5, "none", "returnLastPrediction", False), _max_steps),
}


def mutant(name: str) -> Tuple[Case, dict]:
    key, fn = MUTANTS[name]
    cs = case(*key)
    return cs, fn(cs, _copy(cs.packed[1]))


# --------------------------------------------------------------------------- sibling mixtures (gen_mixture)

MIX_ATOL = 2e-5  # the project's bound for mixture class probabilities (tests/test_mixture_gpu.py)
MIX_NAN_SHARE = 0.25
# (seed, trees, method): weightedConfidence (even seeds) and aggregateNodes (odd), single trees and
# the four ensemble methods
MIXTURES = [(0, 1, "majorityVote"), (1, 1, "majorityVote"), (2, 1, "majorityVote"), (3, 1, "majorityVote"),
            (200, 9, "majorityVote"), (201, 9, "weightedMajorityVote"), (202, 9, "average"),
            (203, 9, "weightedAverage")]


def _from_ir(p) -> tuple:
    from flink_jpmml_amd.pmml import ir

    if isinstance(p, ir.TruePredicate):
        return TRUE
    if isinstance(p, ir.FalsePredicate):
        return FALSE
    if isinstance(p, ir.SimplePredicate):
        return S(p.field, p.operator, p.value)
    if isinstance(p, ir.SimpleSetPredicate):
        return IN(p.field, p.boolean_operator, p.values, "real")
    return C(p.boolean_operator, *[_from_ir(q) for q in p.predicates])


def mixture_forks(compiled, X: np.ndarray) -> Counter:
    """Where the rows' sibling mixtures open, by the PMML rule (the first UNKNOWN child forks the
    walk into itself and every later sibling that is not FALSE): at the ``root``, at ``depth``
    below it on a path that was TRUE so far, or ``inside`` an already open mixture."""
    ev = compiled.evaluator
    trees = [e.tree.root for e in (getattr(ev, "sub", None) or [ev])]
    names = [f"f{j}" for j in range(X.shape[1])]
    w = Walker("none", "returnNullPrediction")
    forks: Counter = Counter()
    for x in X:
        row = {n: float(v) for n, v in zip(names, x)}
        for root in trees:
            if w.ev(_from_ir(root.predicate), row) != T_:
                continue
            stack = [(root, 0, False)]
            while stack:
                node, depth, inside = stack.pop()
                vals = [w.ev(_from_ir(ch.predicate), row) for ch in node.children]
                k = next((i for i, v in enumerate(vals) if v != F_), None)
                if k is None:
                    continue
                if vals[k] == T_:
                    stack.append((node.children[k], depth + 1, inside))
                    continue
                forks["inside" if inside else ("root" if depth == 0 else "depth")] += 1
                stack.extend((ch, depth + 1, True) for ch, v in zip(node.children[k:], vals[k:]) if v != F_)
    return forks


@functools.lru_cache(maxsize=None)
def mixture_case(seed: int, n_trees: int, method: str):
    """``(compiled, X, oracle labels, validity, class probabilities)``: a ``test_mixture_lowering``
    document with numeric labels on cells that sit on its constants +-2 ulps, a quarter of them
    missing."""
    from flink_jpmml_amd.runtime.compiled import CompiledPmml
    from tests.test_mixture_lowering import mixture_doc
    from tests.test_native_walk import NF, VALUES

    doc = mixture_doc(seed, n_trees=n_trees, method=method)
    for k, v in (("a", "1"), ("b", "2"), ("c", "3")):  # as test_mixture_gpu._numeric_labels
        doc = doc.replace(f'value="{k}"', f'value="{v}"').replace(f'score="{k}"', f'score="{v}"')
    c = CompiledPmml.from_string(doc)
    X = np.array(B.boundary_matrix([VALUES] * NF, ROWS, seed))
    X[np.random.default_rng(seed).random(X.shape) < MIX_NAN_SHARE] = np.nan
    X[0] = np.nan
    X[1] = 0.0
    res = c.result(X.astype(np.float64))
    ref, vref = c.score_matrix_oracle(X.astype(np.float64))
    assert np.array_equal(res.valid, vref)
    probs = np.nan_to_num(res.probs)
    for a in (X, ref, vref, probs):
        a.setflags(write=False)
    return c, X, ref, vref, probs


def mixture_clear(probs: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """Valid rows whose two best classes differ by more than twice the tolerance: their label is
    the oracle's whatever the fp32 rounding."""
    top = np.sort(probs, axis=1)
    return valid & (top[:, -1] - top[:, -2] > 2 * MIX_ATOL)
