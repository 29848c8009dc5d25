"""Inputs that sit on a model's own boundaries, and document mutators for the boundary tests.

``boundary_matrix`` fills every cell with one of the column's cuts (split thresholds, interval or
outlier bounds, ...) rounded to fp32 and moved by k in {-2, ..., +2} fp32 ulps, or with a special
value (+-inf, NaN, +-0.0, the smallest subnormal, +-FLT_MAX) — the inputs a random draw never
produces and the only ones on which a wrongly rounded constant or a ``<`` for a ``<=`` shows.

The mutators rewrite ``bench/synth.py`` documents by text (as ``test_gpu_prep_fuzz._treat`` does):
operator pair, child order, decimal thresholds, field data types and integer leaves. With integer
leaves a regression sum (plus the synthetic 0.5 base score) is exact in fp32 in any summation order
while ``|sum| < 2**24``: device and oracle scores are then compared bit for bit, and a single
misrouted walk changes the sum."""

import re
from typing import Callable, Dict, List, Sequence

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
SUBNORMAL = float(np.nextafter(F32(0), F32(1)))
# (value, cells per 64) of the special values; the other 44 of 64 cells hold a cut +- k ulps
SPECIALS = [(np.inf, 4), (-np.inf, 4), (np.nan, 4), (0.0, 2), (-0.0, 2), (SUBNORMAL, 1), (-SUBNORMAL, 1),
            (FLT_MAX, 1), (-FLT_MAX, 1)]
LEAF_PRIME = 251


def ulp_step(x, k: int) -> np.ndarray:
    """fp32 ``x`` moved by ``k`` fp32 ulps (k < 0: down)."""
    x = np.asarray(x, dtype=F32).copy()
    toward = F32(np.inf if k > 0 else -np.inf)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, toward)
    return x


def around(cuts: Sequence[float], ks=(-2, -1, 0, 1, 2)) -> np.ndarray:
    """Every cut rounded to fp32 and moved by each k ulps (fp32, duplicates kept)."""
    base = np.asarray(list(cuts), dtype=np.float64).astype(F32)
    return np.concatenate([ulp_step(base, k) for k in ks]) if len(base) else np.zeros(0, F32)


def boundary_matrix(cuts_per_field: Sequence[Sequence[float]], rows: int, seed: int, specials: bool = True,
                    ks=(-2, -1, 0, 1, 2)) -> np.ndarray:
    """fp32 ``[rows, F]``: per column, fixed shares of cells (``SPECIALS``, per 64) hold the special
    values and every other cell one of the column's cuts rounded to fp32 and moved by k in
    {-2, ..., +2} ulps (cuts and k cycle, so each (cut, k) pair appears as soon as ``rows`` allows);
    the cells of a column are then permuted. No cell holds an ordinary draw."""
    rng = np.random.default_rng(seed)
    X = np.empty((rows, len(cuts_per_field)), dtype=F32)
    for f, cuts in enumerate(cuts_per_field):
        cand = around(sorted(set(float(c) for c in cuts)), ks) if len(cuts) else np.zeros(1, F32)
        col = cand[(np.arange(rows) + 7 * f) % len(cand)].copy()
        if specials:
            kind = np.arange(rows) % 64
            at = 0
            for value, share in SPECIALS:
                col[(kind >= at) & (kind < at + share)] = F32(value)
                at += share
        X[:, f] = col[rng.permutation(rows)]
    return X


# --------------------------------------------------------------------------- reading a document

_PRED = re.compile(r'<SimplePredicate field="([^"]+)" operator="(\w+)" value="([^"]+)"/>')


def split_cuts(txt: str, n_features: int, field_fmt: str = "f{}") -> List[List[float]]:
    """The split constants of every ``SimplePredicate`` per input column."""
    index = {field_fmt.format(j): j for j in range(n_features)}
    cuts: List[Dict[float, None]] = [{} for _ in range(n_features)]
    for name, _, value in _PRED.findall(txt):
        cuts[index[name]][float(value)] = None
    return [list(c) for c in cuts]


# --------------------------------------------------------------------------- mutators


def swap_operator_pair(txt: str) -> str:
    """``lessThan`` / ``greaterOrEqual`` -> ``lessOrEqual`` / ``greaterThan``."""
    return txt.replace('operator="lessThan"', 'operator="lessOrEqual"').replace(
        'operator="greaterOrEqual"', 'operator="greaterThan"')


def rewrite_thresholds(txt: str, fmt: Callable[[float], str]) -> str:
    """Every split constant through ``fmt`` (both predicates of a split share one constant, so they
    stay complementary)."""
    return _PRED.sub(lambda m: f'<SimplePredicate field="{m.group(1)}" operator="{m.group(2)}" '
                               f'value="{fmt(float(m.group(3)))}"/>', txt)


def decimal_thresholds(txt: str) -> str:
    """Two-decimal constants: most are not fp32 numbers, so the lowering has to round them."""
    return rewrite_thresholds(txt, lambda t: f"{t:.2f}")


def integer_thresholds(txt: str) -> str:
    """Integer constants (for ``dataType="integer"`` fields, whose valid inputs are integers)."""
    return rewrite_thresholds(txt, lambda t: f"{int(round(3 * t))}")


def set_data_type(txt: str, data_type: str, fields: Sequence[int] = ()) -> str:
    """``dataType`` of the input fields ``f<j>`` (all of them by default)."""
    which = "|".join(str(j) for j in fields) if len(fields) else r"\d+"
    return re.sub(rf'(<DataField name="f(?:{which})" optype="continuous" dataType=")\w+(")',
                  rf"\g<1>{data_type}\g<2>", txt)


def reverse_children(txt: str) -> str:
    """Both children of every split swapped, so the ``greater...`` child comes first (the ``swap``
    path of ``canonical_threshold``). Node ids and ``defaultChild`` stay as they are."""
    lines = txt.split("\n")

    def node(i: int):
        assert lines[i].lstrip().startswith("<Node"), lines[i]
        if lines[i].rstrip().endswith("</Node>"):
            return [lines[i]], i + 1
        first, j = node(i + 1)
        second, j = node(j)
        assert lines[j].strip() == "</Node>", lines[j]
        return [lines[i]] + second + first + [lines[j]], j + 1

    out, i = [], 0
    while i < len(lines):
        if lines[i].lstrip().startswith("<Node"):
            block, i = node(i)
            out += block
        else:
            out.append(lines[i])
            i += 1
    return "\n".join(out)


def integer_leaves(txt: str, labels: Sequence[str] = (), modulus: int = LEAF_PRIME) -> str:
    """Every leaf ``score`` from a running counter: ``counter % modulus - modulus // 2`` (regression;
    251 by default), or ``labels[counter % len(labels)]`` (votes) — two sibling leaves always
    differ."""
    count = [0]

    def leaf(m):
        k = count[0]
        count[0] += 1
        s = labels[k % len(labels)] if len(labels) else str(k % modulus - modulus // 2)
        return f'{m.group(1)}score="{s}"'

    return re.sub(r'(<Node id="\d+" )score="[^"]+"', leaf, txt)


def null_prediction(txt: str) -> str:
    return txt.replace('missingValueStrategy="defaultChild"', 'missingValueStrategy="nullPrediction"')


def assert_fp32_exact(scores: np.ndarray, valid: np.ndarray) -> None:
    """The oracle's scores are fp32 numbers (integer leaves + 0.5): the bit-exact comparison holds."""
    s = np.asarray(scores, dtype=np.float64)[np.asarray(valid, dtype=bool)]
    assert np.array_equal(s.astype(F32).astype(np.float64), s)
    assert np.all(np.abs(s) < 2 ** 23)  # halves stay exact below 2**23


MUTANTS = {
    "lt": lambda t: t,
    "le": swap_operator_pair,
    "lt-rev": reverse_children,
    "le-rev": lambda t: reverse_children(swap_operator_pair(t)),
    "lt-dec": decimal_thresholds,
    "le-dec": lambda t: swap_operator_pair(decimal_thresholds(t)),
    "le-dec-rev": lambda t: reverse_children(swap_operator_pair(decimal_thresholds(t))),
    "lt-dec-rev": lambda t: reverse_children(decimal_thresholds(t)),
}


def mix_mutants(txt: str) -> str:
    """A different mutant per tree (cycling through ``MUTANTS``), so one document carries both
    operator pairs, both child orders and fp32 as well as decimal thresholds."""
    head, *trees = txt.split("<Segment id=")
    names = list(MUTANTS)
    return head + "".join("<Segment id=" + MUTANTS[names[i % len(names)]](t) for i, t in enumerate(trees))
