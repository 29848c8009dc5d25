"""k-NN classifier documents whose votes are exact in fp32, a float64 reference of the vote that does
not use ``models/knn.py``, and an fp32 twin of ``knn.hip``'s class-output instantiation with mutants.

Exact family. Instances and probe rows lie on ``{0,1}^48`` with unit field weights. Up to four base
points are 32 bits apart (16-bit blocks ``000 / 110 / 101 / 011``); an instance is ``base xor mask``
with a mask of 0, 1, 3, 7 or 15 bits, so its squared-euclidean / cityBlock distance from its base is
that integer and every other base's instances are at least 17 away. A probe row is a base whose group
holds at least ``k`` instances: its ``k`` nearest come from its own group. With ``threshold = 1`` the
weights ``1 / (d + 1)`` are 1, 1/2, 1/4, 1/8, 1/16: every vote total and their sum are multiples of
1/16 up to 32, exact in fp32, and a share is a quotient of two integers <= 512 — never within 2^-53
of an fp32 rounding midpoint, so ``float32(float64 quotient)`` is the correctly rounded fp32 quotient.
With ``threshold = 0`` every probe has an exact match, so the weights are 1 / 0 by the exact-match
rule. :func:`case` asserts this on every row it keeps and drops none.

The other metrics (euclidean, chebychev, minkowski) also rank integer raw sums — their finish is
monotone and ties go to the lower instance index — but their finished distances are not these
integers, so they are used with ``majorityVote`` only; so is the probe row with one missing field (its
distances are rescaled by 48/47).
"""

from __future__ import annotations

import io
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

F = 48
F32 = np.float32
MASK_BITS = (0, 1, 3, 7, 15)
_BLOCKS = ((0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1))
METHODS = {"majority": "majorityVote", "weighted": "weightedMajorityVote"}
EXACT_METRICS = ("squaredEuclidean", "cityBlock")  # their finished distances are the integers
ORDER_METRICS = ("euclidean", "chebychev", 'minkowski p-parameter="3"')  # same neighbours, majorityVote only


def base_point(g: int) -> np.ndarray:
    return np.repeat(np.array(_BLOCKS[g], dtype=np.float64), 16)


def _mask(bits: int, offset: int) -> np.ndarray:
    m = np.zeros(F)
    m[(offset + np.arange(bits)) % F] = 1.0
    return m


def case(groups: Sequence[Sequence[Tuple[int, str]]], k: int, declared: Sequence[str], method: str = "majority",
         metric: str = "squaredEuclidean", threshold: float = 1.0, name: str = "") -> dict:
    """``groups[g]``: the ``(mask bits, target)`` instances around base ``g`` in index order; the
    groups are interleaved round robin into the document's instance order."""
    inst, tgt, grp = [], [], []
    depth = max(len(g) for g in groups)
    for j in range(depth):
        for g, members in enumerate(groups):
            if j < len(members):
                bits, t = members[j]
                assert bits in MASK_BITS
                inst.append(np.abs(base_point(g) - _mask(bits, 5 * j + 3 * g)))
                tgt.append(str(t))
                grp.append(g)
    cats = list(declared)
    for t in tgt:  # a target value the DataField does not declare joins the classes behind the declared ones
        if t not in cats:
            cats.append(t)
    probes = [g for g, members in enumerate(groups) if len(members) >= k]
    assert probes and 1 <= k <= len(inst)
    c = dict(name=name, inst=np.array(inst), targets=tgt, declared=list(declared), categories=cats, k=int(k),
             method=method, metric=metric, threshold=float(threshold), probes=probes,
             weighted=method == "weighted")
    c["exact_rows"] = c["metric"] in EXACT_METRICS
    assert c["exact_rows"] or not c["weighted"], "weighted votes are exact on integer distances only"
    _assert_exact(c)
    return c


def _assert_exact(c: dict) -> None:
    """Every probe base: the k nearest weights are powers of two, or the row has an exact match."""
    for g in c["probes"]:
        d = np.abs(c["inst"] - base_point(g)).sum(axis=1)
        near = np.sort(d, kind="stable")[: c["k"]]
        assert near[-1] <= 15, (c["name"], g, near)
        if not c["weighted"]:
            continue
        if c["threshold"] == 0.0:
            assert near[0] == 0.0, (c["name"], g, "threshold 0 without an exact match")
            continue
        m, _ = np.frexp(1.0 / (near + c["threshold"]))
        assert np.all(m == 0.5), (c["name"], g, near)


def rows(c: dict, n: int) -> np.ndarray:
    """The probe bases (then, for majorityVote, base 0 with field 5 missing; then an all-missing row)
    cycled to ``n`` fp32 rows."""
    pool = [base_point(g) for g in c["probes"]]
    if not c["weighted"]:
        r = base_point(c["probes"][0]).copy()
        r[5] = np.nan
        pool.append(r)
    pool.append(np.full(F, np.nan))
    return np.array([pool[i % len(pool)] for i in range(n)], dtype=F32)


def document(c: dict, outputs: Sequence[str] = (), target_type: str = "string") -> str:
    o = io.StringIO()
    o.write('<?xml version="1.0" encoding="UTF-8"?>\n<PMML xmlns="http://www.dmg.org/PMML-4_4" version="4.4">\n'
            f' <Header description="exact k-NN votes {c["name"]}"/>\n <DataDictionary numberOfFields="{F + 1}">\n')
    for j in range(F):
        o.write(f'  <DataField name="f{j}" optype="continuous" dataType="float"/>\n')
    o.write(f'  <DataField name="y" optype="categorical" dataType="{target_type}">'
            + "".join(f'<Value value="{v}"/>' for v in c["declared"]) + '</DataField>\n </DataDictionary>\n')
    o.write(f' <NearestNeighborModel functionName="classification" numberOfNeighbors="{c["k"]}" '
            f'categoricalScoringMethod="{METHODS[c["method"]]}" threshold="{c["threshold"]!r}">\n'
            '  <MiningSchema>\n   <MiningField name="y" usageType="predicted"/>\n')
    for j in range(F):
        o.write(f'   <MiningField name="f{j}"/>\n')
    o.write('  </MiningSchema>\n')
    if outputs:
        o.write('  <Output>' + "".join(outputs) + '</Output>\n')
    N = len(c["inst"])
    o.write(f'  <TrainingInstances recordCount="{N}" fieldCount="{F + 1}">\n   <InstanceFields>')
    o.write("".join(f'<InstanceField field="f{j}" column="c{j}"/>' for j in range(F)))
    o.write('<InstanceField field="y" column="target"/></InstanceFields>\n   <InlineTable>\n')
    for i in range(N):
        o.write("    <row>" + "".join(f"<c{j}>{int(c['inst'][i, j])}</c{j}>" for j in range(F))
                + f"<target>{c['targets'][i]}</target></row>\n")
    o.write('   </InlineTable>\n  </TrainingInstances>\n'
            f'  <ComparisonMeasure kind="distance"><{c["metric"]}/></ComparisonMeasure>\n  <KNNInputs>')
    o.write("".join(f'<KNNInput field="f{j}"/>' for j in range(F)))
    o.write('</KNNInputs>\n </NearestNeighborModel>\n</PMML>\n')
    return o.getvalue()


def class_outputs(c: dict, target_type: str = "string") -> List[str]:
    """``lab`` / ``shown`` / ``pwin`` / ``p_<class>`` of every class / ``p_nobody`` (a class unknown to the model)."""
    cat = "categorical"
    out = [f'<OutputField name="lab" feature="predictedValue" optype="{cat}" dataType="{target_type}"/>',
           f'<OutputField name="shown" feature="predictedDisplayValue" optype="{cat}" dataType="{target_type}"/>',
           '<OutputField name="pwin" feature="probability" optype="continuous" dataType="double"/>']
    out += [f'<OutputField name="p_{x}" feature="probability" value="{x}" optype="continuous" dataType="double"/>'
            for x in c["categories"][:6]]
    out.append('<OutputField name="p_nobody" feature="probability" value="nobody" optype="continuous" '
               'dataType="double"/>')
    return out


# --------------------------------------------------------------------------- float64 reference


def _distances(c: dict, X: np.ndarray, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """``(finished distance [n, N], row has a present field)``: unit weights, absDiff, missing fields
    skipped and the sum rescaled by F / present (chebychev is not rescaled)."""
    X = np.asarray(X, dtype=dtype)
    C = c["inst"].astype(dtype)
    miss = np.isnan(X)
    v = np.abs(np.where(miss, 0, X)[:, None, :] - C[None, :, :]) * (~miss)[:, None, :]
    present = (~miss).sum(axis=1).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        adj = dtype(F) / present
        met = c["metric"]
        if met == "chebychev":
            return v.max(axis=2), present > 0
        if met.startswith("minkowski"):
            return ((v ** 3).sum(axis=2) * adj[:, None]) ** dtype(1.0 / 3.0), present > 0
        if met == "cityBlock":
            return v.sum(axis=2) * adj[:, None], present > 0
        s = (v * v).sum(axis=2) * adj[:, None]
        return (np.sqrt(s) if met == "euclidean" else s), present > 0


def _vote(c: dict, X: np.ndarray, dtype, mutant: Optional[str] = None):
    """The vote in ``dtype`` arithmetic, rank by rank as the kernel forms it: ``(label index with NaN
    on invalid rows, valid, shares [n, C])``."""
    D, some = _distances(c, X, dtype)
    n, k, cats = len(D), c["k"], c["categories"]
    C = len(cats)
    cls_of = np.array([cats.index(t) for t in c["targets"]])
    if mutant == "swap_classes":
        i, j = 0, next(j for j in range(1, len(cls_of)) if cls_of[j] != cls_of[0])
        cls_of[[i, j]] = cls_of[[j, i]]
    order = np.argsort(np.where(np.isnan(D), np.inf, D), axis=1, kind="stable")[:, :k]
    near = np.take_along_axis(D, order, axis=1)
    valid = some & np.isfinite(near).all(axis=1)
    lab = np.full(n, np.nan)
    shares = np.full((n, C), np.nan, dtype=dtype)
    for r in np.nonzero(valid)[0]:
        cls = cls_of[order[r]]
        if c["weighted"]:
            with np.errstate(divide="ignore"):
                w = (dtype(1.0) / (np.abs(near[r]) + dtype(c["threshold"]))).astype(dtype)
            if np.isinf(w).any() and mutant != "no_exact_rule":
                w = np.isinf(w).astype(dtype)
        else:
            w = np.ones(k, dtype=dtype)
        total = dtype(0)
        for j in range(k):
            total = dtype(total + w[j])
        if mutant == "div_k" and c["weighted"]:
            total = dtype(k)
        shares[r] = 0
        best, best_c = dtype(-1), -1
        for j in range(k):
            v = dtype(0)
            for i in range(k):
                if cls[i] == cls[j]:
                    v = dtype(v + w[i])
            better = v > best or (mutant == "tie_lower_class" and v == best and cls[j] < best_c)
            if better:
                best, best_c = v, cls[j]
            if cls[j] not in cls[:j]:
                col = (cls[j] + 1) % C if mutant == "column_shift" else cls[j]
                with np.errstate(invalid="ignore", divide="ignore"):
                    shares[r, col] = dtype(v) / dtype(total)
        lab[r] = best_c
    return lab, valid, shares


def reference(c: dict, X: np.ndarray):
    """float64: ``(label index, valid, shares [n, C])``."""
    return _vote(c, X, np.float64)


MUTANTS = ("div_k", "no_exact_rule", "tie_lower_class", "swap_classes", "column_shift")


def twin(c: dict, X: np.ndarray, mutant: Optional[str] = None):
    """fp32 twin of the kernel's vote (fp32 weights summed in rank order, fp32 divide)."""
    assert mutant is None or mutant in MUTANTS
    lab, valid, shares = _vote(c, X, np.float32, mutant)
    return lab, valid, shares.astype(F32)


def top_k(shares: np.ndarray, valid: np.ndarray, k: int):
    """Descending, ties to the lower class, -1 / NaN on invalid rows: ``(index int64, share)``."""
    n, C = shares.shape
    idx = np.full((n, k), -1, dtype=np.int64)
    pr = np.full((n, k), np.nan, dtype=shares.dtype)
    for r in np.nonzero(valid)[0]:
        o = sorted(range(C), key=lambda j: (-shares[r, j], j))[:k]
        idx[r, : len(o)] = o
        pr[r, : len(o)] = shares[r, o]
    return idx, pr


def bits(a) -> np.ndarray:
    """fp32 bit patterns with every NaN as one pattern."""
    a = np.ascontiguousarray(np.asarray(a, dtype=F32))
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


# --------------------------------------------------------------------------- the documents

_HAND = [  # k = 5 (targets A B C declared with D, which no instance has; E is not declared)
    [(0, "B"), (1, "A"), (1, "B"), (3, "A"), (3, "C"), (7, "C"), (15, "E")],  # majority: 2-2-1, B ranks first
    [(0, "B"), (1, "A"), (1, "A"), (7, "C"), (7, "C"), (15, "E")],  # weighted: 1 against 1/2 + 1/2, B first
    [(0, "A"), (1, "B"), (1, "C"), (3, "A"), (3, "B"), (3, "E"), (7, "C")],  # ranks 4, 5, 6 tie at d = 3
    [(0, "C"), (0, "E"), (0, "C"), (1, "A"), (1, "A"), (3, "A"), (3, "B")],  # three exact matches
]
_HAND3 = [  # k = 3
    [(0, "B"), (1, "A"), (1, "A"), (3, "C")],  # weighted tie 1 : 1/2 + 1/2
    [(0, "A"), (0, "C"), (1, "C"), (1, "B")],  # two exact matches
    [(0, "E"), (1, "B"), (3, "B"), (3, "A")],  # one exact match, of the undeclared class
]
_DECLARED = ["A", "B", "C", "D"]


def generated(N: int, k: int, C: int, method: str = "majority", metric: str = "squaredEuclidean", seed: int = 0,
              threshold: float = 1.0) -> dict:
    """``N`` instances in as many groups (at most 4) as hold ``k + 1`` each, ``C`` numeric classes ``0 … C-1``
    declared, instance classes drawn at random (every group starts with an exact match)."""
    rng = np.random.default_rng(seed + 7 * N + 13 * k + C)
    G = max(1, min(4, N // (k + 1)))
    sizes = [N // G + (1 if g < N % G else 0) for g in range(G)]
    groups = [[(0 if j == 0 else int(rng.choice(MASK_BITS)), str(int(rng.integers(C)))) for j in range(sz)]
              for sz in sizes]
    return case(groups, k, [str(x) for x in range(C)], method, metric, threshold,
                name=f"n{N}k{k}c{C}_{method}_{metric.split()[0]}")


def _exact_cases() -> Dict[str, dict]:
    out = {}
    for method in ("majority", "weighted"):
        for metric in EXACT_METRICS:
            m = metric[:2]
            out[f"hand5_{method}_{m}"] = case(_HAND, 5, _DECLARED, method, metric, 1.0, f"hand5_{method}_{m}")
            out[f"hand3_t0_{method}_{m}"] = case(_HAND3, 3, _DECLARED, method, metric, 0.0, f"hand3_t0_{method}_{m}")
        out[f"c40k3_{method}"] = generated(65, 3, 40, method, seed=1)
        out[f"n33k9_{method}"] = generated(33, 9, 3, method, "cityBlock", seed=2)
    for metric in ORDER_METRICS:
        out[f"hand5_majority_{metric[:2]}"] = case(_HAND, 5, _DECLARED, "majority", metric, 1.0,
                                                   f"hand5_majority_{metric[:2]}")
    return out


EXACT = _exact_cases()


# --------------------------------------------------------------------------- inexact documents


def inexact() -> Dict[str, dict]:
    """``synth.knn_pmml``: 64 x 4 with k = 5 and 200 x 4 with k = 9, both votes, 3 and 5 classes."""
    from flink_jpmml_amd.bench import synth

    out = {}
    for N, k, classes in ((64, 5, 3), (200, 9, 5)):
        for method in ("majority", "weighted"):
            out[f"knn{N}k{k}_{method}"] = dict(
                text=synth.knn_pmml(N, 4, k=k, method=METHODS[method], classes=classes), k=k, F=4,
                classes=classes, weighted=method == "weighted")
    return out


def inexact_rows(n: int = 1000, F: int = 4) -> np.ndarray:
    return np.random.default_rng(11).standard_normal((n, F)).astype(F32)


def with_outputs(text: str, fields: Sequence[str]) -> str:
    return text.replace("</MiningSchema>", "</MiningSchema>\n  <Output>" + "".join(fields) + "</Output>", 1)
