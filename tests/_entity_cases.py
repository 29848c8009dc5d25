"""Exact documents, probe rows, an independent reference and the twin's mutants for the ranked
entity outputs (``entityId`` / ``clusterId`` / affinity of rank r, the affinity of a named cluster,
the neighbours of a k-NN model).

Integer centres / training instances (``tests/_exact.py::grid_centers``: duplicates 4 and 32 apart,
so exact ties fall inside and across a 32-entity tile and across the two half-waves), field weights
from {0.5, 1, 2}: every raw sum is an exact multiple of 0.5 in both arithmetic forms, and the
float64 oracle, the row-at-a-time reference here, the fp32 twin and the kernel agree in every bit on
rows without a missing field. A missing field brings the Σq/Σq_present rescale, which is not exact:
those rows' affinities are held to 4 fp32 ulps (``docs/PARITY.md``), their ids still to equality.
"""

import io
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from _exact import F32, _num, assert_exact, center_matrix, field_weights, grid_centers
from flink_jpmml_amd.bench.synth import _header

INTERVAL = 40.0  # f0 outside [-INTERVAL, INTERVAL] fails the returnInvalid documents' preparation

# name -> document. ``out``: (feature, rank, value or None, dataType) per Output field, named o0, o1 ...
_AFF = "affinity"


def _ranked(ranks: Sequence[int], id_type: str = "string", cluster_id: bool = False) -> List[tuple]:
    out = []
    for r in ranks:
        out.append(("entityId", r, None, id_type))
        out.append((_AFF, r, None, "double"))
        if cluster_id:
            out.append(("clusterId", r, None, "integer"))
    return out


CASES: Dict[str, dict] = {
    # clustering: K, F, metric, Output fields
    "c1x1": dict(kind="cluster", N=1, F=1, metric="squaredEuclidean", out=_ranked((1, 2), cluster_id=True)),
    "c2x5": dict(kind="cluster", N=2, F=5, metric="euclidean", out=_ranked((1, 2, 3), "integer")),
    "c9x5_named": dict(kind="cluster", N=9, F=5, metric="squaredEuclidean", name_all=True,
                       out=_ranked((1, 2, 8)) + [("predictedValue", 1, None, "string")]),
    "c31x1_city": dict(kind="cluster", N=31, F=1, metric="cityBlock", out=_ranked((1, 2, 8), cluster_id=True)),
    "c9x5_cheby": dict(kind="cluster", N=9, F=5, metric="chebychev", out=_ranked((2, 3))),
    "c32x64": dict(kind="cluster", N=32, F=64, metric="squaredEuclidean", out=_ranked((1, 9, 32), "integer")),
    "c33x5_interval": dict(kind="cluster", N=33, F=5, metric="euclidean", interval=True, name=(3, 7),
                           out=_ranked((1, 2, 8))),
    "c65x5": dict(kind="cluster", N=65, F=5, metric="euclidean", out=_ranked((9, 32), cluster_id=True)),
    # k-NN: N, F, k, metric, instanceIdVariable, Output fields
    "k5n33_ids": dict(kind="knn", N=33, F=5, k=5, metric="squaredEuclidean", id_var=True,
                      out=[("predictedValue", 1, None, "double")] + _ranked((1, 2, 3, 4, 5, 6))),
    "k8n65_rows": dict(kind="knn", N=65, F=5, k=8, metric="euclidean", id_var=False, interval=True,
                       out=_ranked((1, 2, 8), "integer")),
    "k32n65x64": dict(kind="knn", N=65, F=64, k=32, metric="squaredEuclidean", id_var=True,
                      out=_ranked((9, 32))),
    "k2n2": dict(kind="knn", N=2, F=1, k=2, metric="cityBlock", id_var=True, out=_ranked((1, 2, 3))),
    "k1n9": dict(kind="knn", N=9, F=5, k=1, metric="squaredEuclidean", id_var=True,
                 out=_ranked((1, 2)) + [("predictedValue", 1, None, "double")]),
}
MFMA_CASES = [n for n, c in CASES.items() if c["metric"] in ("squaredEuclidean", "euclidean")]


def entities(case: dict, seed: int = 5) -> Tuple[np.ndarray, np.ndarray]:
    """``(C [N, F] integer centres / instances, w [F] field weights)``."""
    C = grid_centers(case["N"], case["F"], seed=seed)
    if len(C) > 6:
        C[6] = C[2]  # the other half-wave of the same tile
    if len(C) > 34:
        C[34] = C[2]  # the next tile: a three-way tie with 2 and 6
    return C, field_weights(case["F"], seed)


def instance_ids(case: dict) -> List[str]:
    """What ``entityId`` must answer: the instanceIdVariable column (``i<row>`` strings, or the
    numbers 100 + 3 row for an integer field), 1-based row numbers without one, cluster ids ``k + 1``."""
    N = case["N"]
    if case["kind"] == "cluster" or not case.get("id_var"):
        return [str(i + 1) for i in range(N)]
    integer = any(o[0] == "entityId" and o[3] == "integer" for o in case["out"])
    return [str(100 + 3 * i) if integer else f"i{i}" for i in range(N)]


def targets(case: dict) -> np.ndarray:
    """Regression targets of the k-NN documents: distinct from every id."""
    return 1000.0 + 2.0 * np.arange(case["N"])


def outputs(case: dict) -> List[tuple]:
    """``(name, feature, rank, value, dataType)`` of every Output field, the named clusters last."""
    out = [(f"o{i}",) + tuple(o) for i, o in enumerate(case["out"])]
    named = range(case["N"]) if case.get("name_all") else case.get("name", ())
    out += [(f"n{k}", _AFF, 1, str(k + 1), "double") for k in named]
    return out


def document(case: dict, seed: int = 5) -> str:
    C, w = entities(case, seed)
    N, F = C.shape
    o = io.StringIO()
    _header(o, f"exact entity ranks {case['kind']} {N} x {F}")
    o.write(f' <DataDictionary numberOfFields="{F + 1}">\n')
    for j in range(F):
        iv = f'<Interval closure="closedClosed" leftMargin="{-INTERVAL}" rightMargin="{INTERVAL}"/>' \
            if case.get("interval") and j == 0 else ""
        o.write(f'  <DataField name="f{j}" optype="continuous" dataType="float">{iv}</DataField>\n')
    knn = case["kind"] == "knn"
    o.write(f'  <DataField name="y" optype="{"continuous" if knn else "categorical"}" '
            f'dataType="{"double" if knn else "string"}"/>\n </DataDictionary>\n')
    if knn:
        o.write(f' <NearestNeighborModel functionName="regression" numberOfNeighbors="{case["k"]}" '
                f'continuousScoringMethod="average">\n')
    else:
        o.write(f' <ClusteringModel modelName="probe" functionName="clustering" modelClass="centerBased" '
                f'numberOfClusters="{N}">\n')
    o.write('  <MiningSchema>\n   <MiningField name="y" usageType="predicted"/>\n')
    for j in range(F):
        ivt = ' invalidValueTreatment="returnInvalid"' if case.get("interval") and j == 0 else ""
        o.write(f'   <MiningField name="f{j}"{ivt}/>\n')
    o.write('  </MiningSchema>\n  <Output>\n')
    for name, feat, rank, value, dtype in outputs(case):
        val = f' value="{value}"' if value is not None else ""
        optype = "continuous" if dtype == "double" else "categorical"
        o.write(f'   <OutputField name="{name}" feature="{feat}" rank="{rank}"{val} optype="{optype}" '
                f'dataType="{dtype}"/>\n')
    o.write('  </Output>\n')
    measure = f'  <ComparisonMeasure kind="distance"><{case["metric"]}/></ComparisonMeasure>\n'
    if knn:
        ids = instance_ids(case)
        idv = ' instanceIdVariable="rowid"' if case.get("id_var") else ""
        o.write(f'  <TrainingInstances recordCount="{N}" fieldCount="{F + 2}"{idv}>\n   <InstanceFields>')
        o.write("".join(f'<InstanceField field="f{j}" column="c{j}"/>' for j in range(F)))
        o.write('<InstanceField field="y" column="target"/>')
        if case.get("id_var"):
            o.write('<InstanceField field="rowid" column="rid"/>')
        o.write('</InstanceFields>\n   <InlineTable>\n')
        y = targets(case)
        for i in range(N):
            rid = f"<rid>{ids[i]}</rid>" if case.get("id_var") else ""
            o.write("    <row>" + "".join(f"<c{j}>{_num(C[i, j])}</c{j}>" for j in range(F))
                    + f"<target>{_num(y[i])}</target>{rid}</row>\n")
        o.write('   </InlineTable>\n  </TrainingInstances>\n' + measure + '  <KNNInputs>')
        o.write("".join(f'<KNNInput field="f{j}" fieldWeight="{_num(w[j])}"/>' for j in range(F)))
        o.write('</KNNInputs>\n </NearestNeighborModel>\n</PMML>\n')
    else:
        o.write(measure)
        for j in range(F):
            o.write(f'  <ClusteringField field="f{j}" compareFunction="absDiff" fieldWeight="{_num(w[j])}"/>\n')
        for k in range(N):
            o.write(f'  <Cluster id="{k + 1}" name="c{k + 1}"><Array n="{F}" type="real">'
                    + " ".join(_num(v) for v in C[k]) + '</Array></Cluster>\n')
        o.write(' </ClusteringModel>\n</PMML>\n')
    return o.getvalue()


def probe_rows(case: dict, rows: int = 48, seed: int = 5) -> np.ndarray:
    """``center_matrix``: grid rows with a NaN here and there and row 16 all missing, every entity
    itself (on a centre; two- and three-way ties through the duplicates), the shadowed entities moved
    one step; then one row outside the returnInvalid interval."""
    C, _ = entities(case, seed)
    X = center_matrix(C, rows, seed=seed, nan_every=7)
    bad = X[1].copy()
    bad[0] = INTERVAL + 8.0
    return np.concatenate([X, bad[None, :]]).astype(F32)


def take_rows(X: np.ndarray, n: int) -> np.ndarray:
    """``n`` rows of ``X``, cycled: the batch sizes around the 64-row and 256-row tile edges."""
    return X[np.arange(n) % len(X)]


# --------------------------------------------------------------------------- row-at-a-time reference


def reference(case: dict, X: np.ndarray, lookup, seed: int = 5, guard: bool = True) -> Dict[str, np.ndarray]:
    """Every Output column of ``case`` in float64, one row at a time from the builder's own arrays:
    raw sums over the present fields, the rescale, the root, a sort by (distance, entity index).
    ``lookup(name, id string) -> float`` is the schema's encoding of an id for a field."""
    C, w = entities(case, seed)
    N, F = C.shape
    metric, knn = case["metric"], case["kind"] == "knn"
    ids = instance_ids(case)
    limit = min(case["k"], N) if knn else min(N, 32)
    cols = {o[0]: np.full(len(X), np.nan) for o in outputs(case)}
    raws = []
    for r, x in enumerate(np.asarray(X, dtype=np.float64)):
        pres = ~np.isnan(x)
        if case.get("interval") and pres[0] and abs(x[0]) > INTERVAL:
            continue
        if not pres.any():
            continue
        dist = []
        for i in range(N):
            d = np.abs(x[pres] - C[i][pres])
            if metric in ("squaredEuclidean", "euclidean"):
                s = float(np.sum(w[pres] * d * d))
            elif metric == "cityBlock":
                s = float(np.sum(w[pres] * d))
            else:
                s = float(np.max(w[pres] * d))
            raws.append(s)
            if metric != "chebychev":
                s = s * (F / pres.sum())
            dist.append(float(np.sqrt(s)) if metric == "euclidean" else s)
        order = sorted(range(N), key=lambda i: (dist[i], i))
        y = float(np.mean(targets(case)[order[:limit]])) if knn else None
        for name, feat, rank, value, _ in outputs(case):
            if feat == "predictedValue":
                cols[name][r] = y if knn else lookup(name, ids[order[0]])
            elif value is not None:
                cols[name][r] = dist[int(value) - 1]
            elif rank > limit:
                continue
            elif feat == "entityId":
                cols[name][r] = lookup(name, ids[order[rank - 1]])
            elif feat == "clusterId":
                cols[name][r] = order[rank - 1] + 1.0
            else:
                cols[name][r] = dist[order[rank - 1]]
    if guard:
        assert_exact([np.array(raws)], dyadic=0.5)
    return cols


def complete_rows(X: np.ndarray) -> np.ndarray:
    return ~np.isnan(np.asarray(X, dtype=np.float64)).any(axis=1)


def ulps(got, want) -> np.ndarray:
    """Distance in fp32 ulps of ``want`` (NaN against NaN: 0; NaN against a number: inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    return np.where(both, 0.0, np.where(np.isnan(d), np.inf, d))


def assert_columns(case: dict, got: Dict[str, np.ndarray], want: Dict[str, np.ndarray], X: np.ndarray, what) -> None:
    """fp32 ``got`` against float64 ``want``: ids equal on every row; affinities equal in every bit on
    complete rows (the float64 value rounds once to fp32) and within 4 ulps on rows with a missing field."""
    full = complete_rows(X)
    for name, feat, _, _, _ in outputs(case):
        g = np.asarray(got[name], dtype=F32)
        w32 = np.asarray(want[name], dtype=np.float64).astype(F32)
        if feat != _AFF:
            assert np.array_equal(g, w32, equal_nan=True), (what, name, np.flatnonzero(~((g == w32) | (g != g) & (w32 != w32)))[:8])
            continue
        assert np.array_equal(g[full].view(np.uint32), w32[full].view(np.uint32)), \
            (what, name, np.flatnonzero(g[full].view(np.uint32) != w32[full].view(np.uint32))[:8])
        worst = ulps(g[~full], want[name][~full])
        assert not worst.size or worst.max() <= 4.0, (what, name, float(worst.max()))


# --------------------------------------------------------------------------- mutants of the twin


def mutants() -> Dict[str, dict]:
    """Named single-rule changes of ``ops/entities.py`` (attribute -> replacement). Every one must
    show on some exact document."""
    from flink_jpmml_amd.ops import entities as E

    def offer_late(ck, worst):
        with np.errstate(invalid="ignore"):
            return ck <= worst

    def before_high(ck, ci, kj, ij):
        with np.errstate(invalid="ignore"):
            return (ck < kj) | ((ck == kj) & (ci > ij) & (ij != 0x7FFFFFFF))

    def unfinished(T, s, adj):
        return np.asarray(s, dtype=F32)

    def named_swapped(T, e):
        nxt = [int(v) for v in T.named if v >= 0]
        cur = int(T.named[e])
        return nxt[(nxt.index(cur) + 1) % len(nxt)] if cur >= 0 and len(nxt) > 1 else cur

    def no_merge(key0, id0, key1, id1, k):
        return None

    return {
        "ties to the higher index": {"_offer": offer_late, "_before": before_high},
        "unfinished affinity": {"_finish": unfinished},
        "rank off by one": {"_rank": lambda arg: arg + 1},
        "named column swapped": {"_named_column": named_swapped},
        "half-wave merge dropped": {"_merge": no_merge},
    }, E


# --------------------------------------------------------------------------- inexact inputs

TOL = 2e-5  # rtol = atol of the fp32 distance sums (tests/test_gpu_kernels.py)


def with_ranked_outputs(text: str, ranks: Sequence[int], named: Sequence[str] = ()) -> str:
    """``text`` (a ``bench/synth.py`` clustering or k-NN document) with ``id<r>`` (clusterId: the
    1-based entity position, whatever the ids are) and ``aff<r>`` Output fields of every rank, and
    ``named<id>`` affinities of the named clusters."""
    knn = "NearestNeighborModel" in text
    fields = []
    for r in ranks:
        feat = "entityId" if knn else "clusterId"
        fields.append(f'<OutputField name="id{r}" feature="{feat}" rank="{r}" optype="categorical" dataType="integer"/>')
        fields.append(f'<OutputField name="aff{r}" feature="affinity" rank="{r}" optype="continuous" dataType="double"/>')
    for v in named:
        fields.append(f'<OutputField name="named{v}" feature="affinity" value="{v}" optype="continuous" '
                      f'dataType="double"/>')
    return text.replace("</MiningSchema>", "</MiningSchema>\n  <Output>" + "".join(fields) + "</Output>", 1)


def _inexact() -> Dict[str, dict]:
    from flink_jpmml_amd.bench import synth

    km = synth.kmeans_pmml
    return {
        "kmeans9x4": dict(text=with_ranked_outputs(km(9, 4, seed=3), (1, 2, 3), ("2", "9")), F=4, ranks=(1, 2, 3),
                          mfma=True),
        "kmeans33x8_euclid": dict(text=with_ranked_outputs(km(33, 8, seed=4, metric="euclidean", weighted=True),
                                                           (1, 2, 8)), F=8, ranks=(1, 2, 8), mfma=True),
        "kmeans65x8_city": dict(text=with_ranked_outputs(km(65, 8, seed=5, metric="cityBlock"), (1, 9)), F=8,
                                ranks=(1, 9)),
        "kmeans9x4_minkowski": dict(text=with_ranked_outputs(km(9, 4, seed=6, metric='minkowski p-parameter="3"'),
                                                             (1, 2)), F=4, ranks=(1, 2), transcendental=True),
        "kmeans9x4_gauss": dict(text=with_ranked_outputs(km(9, 4, seed=7, compare="gaussSim")
                                                         .replace('kind="distance"', 'kind="similarity"'), (1, 2)),
                                F=4, ranks=(1, 2), transcendental=True),
        "knn64x4": dict(text=with_ranked_outputs(synth.knn_pmml(64, 4, k=5, classification=False, seed=2),
                                                 (1, 2, 5)), F=4, ranks=(1, 2, 5), mfma=True),
    }


INEXACT = _inexact()


def inexact_tolerance(spec: dict) -> float:
    """rtol = atol of the affinities of ``spec`` against the float64 oracle."""
    return TOL


def inexact_rows(spec: dict, rows: int = 1000) -> np.ndarray:
    from flink_jpmml_amd.bench.synth import stream_matrix

    return stream_matrix(rows, spec["F"], seed=11, missing_rate=0.01)


def oracle_measure(compiled, X: np.ndarray):
    """``(D float64 [n, N], key [n, N] ascending = nearer, NaN last)`` of the prepared rows."""
    P, _ = compiled.prepare(np.asarray(X, dtype=np.float64))
    ev = compiled.evaluator
    D = ev.distances(ev.feature_matrix(compiled.columns(P)))
    return D, np.where(np.isnan(D), np.inf, D if ev.kind_distance else -D)


def undecided(compiled, X: np.ndarray, ranks: Sequence[int], tol: float = TOL) -> np.ndarray:
    """bool ``[len(ranks), n]``: rows whose rank r the oracle does not decide for an fp32 kernel —
    a gap to rank r - 1 or r + 1 that is neither an exact tie nor at least twice the tolerance."""
    _, key = oracle_measure(compiled, X)
    srt = np.sort(key, axis=1)
    out = np.zeros((len(ranks), len(X)), dtype=bool)
    for j, r in enumerate(ranks):
        for a, b in ((r - 2, r - 1), (r - 1, r)):
            if a < 0 or b >= srt.shape[1]:
                continue
            with np.errstate(invalid="ignore"):
                gap = srt[:, b] - srt[:, a]
                need = 2.0 * (tol + tol * np.maximum(np.abs(srt[:, a]), np.abs(srt[:, b])))
                out[j] |= (gap > 0) & (gap < need)
    return out


__all__ = ["CASES", "MFMA_CASES", "assert_columns", "complete_rows", "document", "entities", "instance_ids",
           "mutants", "outputs", "probe_rows", "reference", "take_rows", "targets", "ulps"]
