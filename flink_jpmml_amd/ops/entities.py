"""Ranked entities of the distance families on the device (``csrc/entities.hip``) and its numpy twin.

``entities_launch`` launches ``pmml_entities_launch`` over the raw rows a ``ClusterPlan`` /
``KnnPlan`` scored. An :class:`EntityTables` holds the distance model in the plan's own fp32 tensors
and the column program:

==============  ==============================================================================
``ent``         ``float32 [N, F]`` centres / training instances
``weights``     ``float32 [F]``; ``scales`` (gaussSim), ``qweights`` (missing-value weights) alike
``cfun``        ``int32 [F]`` compare function codes (absDiff, gaussSim, delta, equal)
``wc``, ``cc``  the expansion's operands (``ClusterPlan.mfma_operands``), or None: the VALU form
``cols``        ``int32 [n_col, 4]`` ``{op, arg, table offset, destination column}``
``named``       ``int32 [N]``: the tile column (index into ``cols``) of the first field naming the
                entity, -1 for none
``tables``      ``float32``: per ``ENT_ID`` column the encodings of the ``N`` entity ids
==============  ==============================================================================

``ENT_ID`` (arg = 0-based rank) writes ``tables[offset + entity]``, ``ENT_AFFINITY`` (arg = rank) the
finished distance or similarity, ``ENT_NAMED`` (arg = entity) that entity's. ``k`` is the length of
the list: the largest rank asked of a ClusteringModel, the ``k`` of a NearestNeighborModel.
``knn`` selects whose arithmetic is repeated (``entities.hip`` header): 0 compares finished values
as ``cluster_kernel`` does, 1 raw sums as ``knn_kernel`` does; the expansion clamps at 0 after
(``cluster_mfma_kernel``) or before (``knn_mfma_kernel``) the comparison.

A row is valid when no field preparation rejected it, some field is present (``Σq_present > 0``)
and rank 1 is finite (``knn``: all ``k`` neighbours are). Invalid rows, ranks past the list and
entries with a non-finite affinity are NaN.

``entities_numpy`` repeats the kernel statement by statement in fp32 (``fmaf`` as one float64
multiply-add rounded to fp32: exact whenever the fp32 result is, which is all the exact probes ask).
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from .reasons import (FP_CODE_RANGE, FP_HAS_INTERVAL, FP_HI_OPEN, FP_INTEGER, FP_INVALID_RETURN, FP_LO_OPEN,
                      FP_MISSING_VALUE, FP_ROW_INVALID, FP_VALUE_LIST, FP_VALUE_MASK, prep_numpy)

ENT_ID, ENT_AFFINITY, ENT_NAMED = 0, 1, 2
M_SQEUCLID, M_EUCLID, M_CITY, M_CHEBY, M_MINKOWSKI = range(5)
CF_ABSDIFF, CF_GAUSS, CF_DELTA, CF_EQUAL = range(4)

MAX_RANK = 32
MAX_COLUMNS = 64
MAX_FEATURES = 128
LDS_BYTES = 64 * 1024  # one workgroup's request: two workgroups share a CU's 160 KiB
ROWS = (256, 128, 64)  # rows (= lanes) of one workgroup, the first that fits

_f32 = np.float32
_EMPTY_ID = 0x7FFFFFFF


def template_k(k: int) -> int:
    """The kernel instantiation (8 or 32 list registers) that holds ``k`` entries."""
    if not 1 <= k <= MAX_RANK:
        raise ValueError(f"entity rank must be in [1, {MAX_RANK}], got {k}")
    return 8 if k <= 8 else 32


def lds_bytes(n_feat: int, n_col: int, rows: int) -> int:
    """LDS request of one workgroup (``entities.hip`` ``ent_lds_bytes``): the ``[F][rows]`` feature
    planes, the rejected flags and the ``[rows][n_col | 1]`` output tile."""
    return n_feat * rows * 4 + rows * 4 + rows * (n_col | 1) * 4


def geometry(n_feat: int, n_col: int) -> int:
    """Rows per workgroup: 256, 128 or 64, the first whose request fits ``LDS_BYTES``."""
    for rows in ROWS:
        if lds_bytes(n_feat, n_col, rows) <= LDS_BYTES:
            return rows
    raise ValueError(f"{n_feat} fields and {n_col} columns need {lds_bytes(n_feat, n_col, 64)} bytes of LDS "
                     f"for 64 rows > {LDS_BYTES}")


class EntityTables:
    """The distance model and the column program (module docstring), checked once: every index a
    lane follows stays inside its table and every destination column inside the matrix."""

    def __init__(self, ent, weights, scales, qweights, cfun, metric: int, similarity: bool, p: float, cols, named,
                 tables, k: int, knn: bool, width: int, wc=None, cc=None):
        self.ent = np.ascontiguousarray(ent, dtype=np.float32)
        self.weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        self.scales = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
        self.qweights = np.ascontiguousarray(qweights, dtype=np.float32).reshape(-1)
        self.cfun = np.ascontiguousarray(cfun, dtype=np.int32).reshape(-1)
        self.metric, self.similarity, self.p = int(metric), bool(similarity), float(p)
        self.cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1, 4)
        self.named = np.ascontiguousarray(named, dtype=np.int32).reshape(-1)
        self.tables = np.ascontiguousarray(tables if len(tables) else [0.0], dtype=np.float32).reshape(-1)
        self.k, self.knn, self.width = int(k), bool(knn), int(width)
        self.wc = None if wc is None else np.ascontiguousarray(wc, dtype=np.float32)
        self.cc = None if cc is None else np.ascontiguousarray(cc, dtype=np.float32).reshape(-1)
        self._check()
        self.n_ent, self.n_feat = (int(v) for v in self.ent.shape)
        self.rows = geometry(self.n_feat, len(self.cols))
        self._device = {}

    @property
    def variant(self) -> str:
        return "valu" if self.wc is None else "mfma"

    def _check(self) -> None:
        if self.ent.ndim != 2 or self.ent.shape[0] < 1 or not 1 <= self.ent.shape[1] <= MAX_FEATURES:
            raise ValueError(f"entity kernel handles [N >= 1, 1 .. {MAX_FEATURES}] entities, got {self.ent.shape}")
        N, F = self.ent.shape
        if any(len(v) != F for v in (self.weights, self.scales, self.qweights, self.cfun)) or len(self.named) != N:
            raise ValueError("entity tables: a per-field or per-entity table has the wrong length")
        if not M_SQEUCLID <= self.metric <= M_MINKOWSKI or ((self.cfun < 0) | (self.cfun > CF_EQUAL)).any():
            raise ValueError("entity tables: unknown metric or compare function")
        if not 1 <= self.k <= min(N, MAX_RANK):
            raise ValueError(f"entity kernel keeps 1 .. min(N, {MAX_RANK}) entries, got k = {self.k}")
        c = self.cols
        if not 1 <= len(c) <= MAX_COLUMNS or self.width < 1:
            raise ValueError(f"entity kernel writes 1 .. {MAX_COLUMNS} columns")
        if ((c[:, 0] < ENT_ID) | (c[:, 0] > ENT_NAMED)).any() or ((c[:, 3] < 0) | (c[:, 3] >= self.width)).any():
            raise ValueError("entity tables: a column's op or destination is out of range")
        if len(set(c[:, 3].tolist())) != len(c):
            raise ValueError("entity tables: two columns share a destination")
        ranked = c[:, 0] != ENT_NAMED
        if (c[ranked, 1] < 0).any() or (c[ranked, 1] >= MAX_RANK).any():
            raise ValueError(f"entity tables: a rank outside 1 .. {MAX_RANK}")
        ids = c[:, 0] == ENT_ID
        if ((c[ids, 2] < 0) | (c[ids, 2] + N > self.tables.size)).any():
            raise ValueError("entity tables: an id table lies outside the tables")
        for j in np.flatnonzero(~ranked):
            e = int(c[j, 1])
            if not 0 <= e < N or not 0 <= self.named[e] <= j or c[self.named[e], 0] != ENT_NAMED \
                    or c[self.named[e], 1] != e:
                raise ValueError("entity tables: a named column and the named table disagree")
        if ((self.named < -1) | (self.named >= len(c))).any():
            raise ValueError("entity tables: the named table points outside the columns")
        for e in np.flatnonzero(self.named >= 0):
            if c[self.named[e], 0] != ENT_NAMED or c[self.named[e], 1] != e:
                raise ValueError("entity tables: the named table points at another column")
        if (self.wc is None) != (self.cc is None):
            raise ValueError("entity tables: wc and cc come together")
        if self.wc is not None:
            Np, Fp = self.wc.shape
            if Np % 32 or Fp % 2 or Fp < F or Np < N or len(self.cc) != Np or self.similarity \
                    or self.metric not in (M_SQEUCLID, M_EUCLID) or (self.cfun != CF_ABSDIFF).any():
                raise ValueError("entity tables: the expansion needs squared / plain euclidean absDiff distances "
                                 "and operands padded to the 32 x 2 tile")

    def on(self, device):
        """The tables as device tensors (cached per device)."""
        import torch

        key = str(device)
        d = self._device.get(key)
        if d is None:
            names = ["ent", "weights", "scales", "qweights", "cfun", "cols", "named", "tables"]
            names += ["wc", "cc"] if self.wc is not None else []
            d = self._device[key] = {k: torch.from_numpy(getattr(self, k)).to(device) for k in names}
        return d


def entities_launch(X, out, tables: EntityTables, prep=None, rows: Optional[int] = None, stream=None) -> None:
    """Device tensors: ``X`` fp32 ``[m, n_feat]`` (unit column stride, any row stride), ``out`` fp32
    ``[m, width]`` (unit column stride, any row stride): only the columns ``tables.cols`` names are
    written. ``prep``: the int32 ``FieldPrep`` table of the raw rows or None. ``rows`` overrides
    :func:`geometry`."""
    from . import _lib

    T = tables
    m = int(X.shape[0])
    if X.dim() != 2 or int(X.shape[1]) != T.n_feat or (T.n_feat > 1 and X.stride(1) != 1) \
            or (m > 1 and X.stride(0) < T.n_feat):
        raise ValueError(f"entities_launch needs a row-major [m, {T.n_feat}] X with unit column stride")
    if out.dim() != 2 or int(out.shape[0]) != m or int(out.shape[1]) != T.width \
            or (T.width > 1 and out.stride(1) != 1) or (m > 1 and out.stride(0) < T.width):
        raise ValueError(f"entities_launch needs a row-major [m, {T.width}] out with unit column stride")
    if prep is not None and (not prep.is_contiguous() or int(prep.numel()) < 8 * T.n_feat):
        raise ValueError("entities_launch needs a contiguous FieldPrep table of n_feat records")
    rows = T.rows if rows is None else int(rows)
    if rows not in ROWS or lds_bytes(T.n_feat, len(T.cols), rows) > LDS_BYTES:
        raise ValueError(f"entities_launch: {rows} rows per workgroup do not fit {LDS_BYTES} bytes of LDS")
    d = T.on(X.device)
    a = _lib.EntityArgs()
    a.X, a.prep = X.data_ptr(), (prep.data_ptr() if prep is not None else None)
    a.ent, a.weights, a.scales = d["ent"].data_ptr(), d["weights"].data_ptr(), d["scales"].data_ptr()
    a.qweights, a.cfun = d["qweights"].data_ptr(), d["cfun"].data_ptr()
    a.wc = d["wc"].data_ptr() if T.wc is not None else None
    a.cc = d["cc"].data_ptr() if T.wc is not None else None
    a.cols, a.named, a.tables, a.out = d["cols"].data_ptr(), d["named"].data_ptr(), d["tables"].data_ptr(), out.data_ptr()
    a.n_rows, a.n_feat = m, T.n_feat
    a.ldx = int(X.stride(0)) if m > 1 else T.n_feat
    a.ldo = int(out.stride(0)) if m > 1 else T.width
    a.n_ent, a.metric, a.similarity, a.k = T.n_ent, T.metric, int(T.similarity), T.k
    a.knn, a.n_col, a.n_tables, a.rows = int(T.knn), len(T.cols), int(T.tables.size), rows
    a.Np, a.Fp = (int(v) for v in T.wc.shape) if T.wc is not None else (0, 0)
    a.p = T.p
    _lib.check(_lib.load().pmml_entities_launch(_lib.stream_handle(stream), a), "pmml_entities_launch")


# --------------------------------------------------------------------------- numpy twin


def prep_bad_numpy(x: np.ndarray, prep: np.ndarray, f: int) -> np.ndarray:
    """The rows ``common.h::prep_value`` rejects for column ``f`` (``*bad``): an invalid value under
    ``returnInvalid``, or a field whose definition rejects every value."""
    x = np.asarray(x, dtype=np.float32)
    raw = np.asarray(prep).view(np.uint32).reshape(-1, 8)
    rec = raw[f]
    fl = int(rec[0])
    if fl == 0:
        return np.zeros(len(x), dtype=bool)
    if fl & FP_ROW_INVALID:
        return np.ones(len(x), dtype=bool)
    if not fl & FP_INVALID_RETURN:
        return np.zeros(len(x), dtype=bool)
    lo, hi, _, _, _, _, pad = (np.float32(v) for v in rec[1:8].view(np.float32))
    with np.errstate(invalid="ignore"):
        miss = x != x
        if fl & FP_MISSING_VALUE:
            miss |= x == pad
        invalid = np.zeros(len(x), dtype=bool)
        if fl & FP_VALUE_LIST:
            w = int(rec[7])
            vlist = raw.reshape(-1).view(np.float32)[8 * f + (w & 0xFFFF):]
            n_miss, n_inv = (w >> 16) & 0xFF, w >> 24
            for i in range(n_miss):
                miss |= x == vlist[i]
            for i in range(n_inv):
                invalid |= x == vlist[n_miss + i]
        if fl & FP_HAS_INTERVAL:
            lo_ok = (x > lo) if fl & FP_LO_OPEN else (x >= lo)
            hi_ok = (x < hi) if fl & FP_HI_OPEN else (x <= hi)
            invalid |= ~(lo_ok & hi_ok)
        if fl & FP_CODE_RANGE:
            invalid |= ~((x >= 0) & (x < hi))
        if fl & FP_INTEGER:
            invalid |= np.floor(x) != x
        if fl & FP_VALUE_MASK:
            d = (x - lo).astype(np.float32)
            inside = (d >= 0) & (d < 64) & (np.floor(x) == x)
            bits = int(rec[5]) | (int(rec[6]) << 32)
            inside &= np.array([(bits >> int(v)) & 1 for v in np.where(inside, d, 0).astype(np.int64)], dtype=bool)
            invalid |= ~inside
    return invalid & ~miss


def _fma(a, b, c):
    """``fmaf``: the product is exact in float64; one rounding to fp32 whenever the float64 sum is exact."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
            + np.asarray(c, dtype=np.float64)).astype(_f32)


# The rules the tests' mutants replace one at a time.


def _offer(ck, worst):
    """A candidate enters the list when it beats the k-th key: strict, an equal key arriving later
    (a higher index) stays out."""
    with np.errstate(invalid="ignore"):
        return ck < worst


def _before(ck, ci, kj, ij):
    """List order: the smaller key, then the lower entity index."""
    with np.errstate(invalid="ignore"):
        return (ck < kj) | ((ck == kj) & (ci < ij))


def _finish(T: EntityTables, s, adj):
    """``finish_distance``: rescale (not chebychev), root (euclidean), 1/p power (minkowski)."""
    s = np.asarray(s, dtype=_f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if T.metric != M_CHEBY:
            s = (s * adj).astype(_f32)
        if T.metric == M_EUCLID:
            s = np.sqrt(np.where(s > 0, s, _f32(0))).astype(_f32)  # fmaxf(s, 0): NaN -> 0
        elif T.metric == M_MINKOWSKI:
            s = np.power(s, _f32(1.0) / _f32(T.p)).astype(_f32)
    return s


def _rank(arg: int) -> int:
    """The list slot of a column's 0-based rank."""
    return arg


def _named_column(T: EntityTables, e: int) -> int:
    """The tile column that takes entity ``e``'s affinity."""
    return int(T.named[e])


def _merge(key0, id0, key1, id1, k: int):
    """The lane^32 merge: the partner half-wave's entries offered to this lane's list in order."""
    for j in range(k):
        o, p = key1[:, j].copy(), id1[:, j].copy()
        wk = key0[:, :k].max(axis=1)
        wi = np.where(key0[:, :k] == wk[:, None], id0[:, :k], -1).max(axis=1)
        _insert(key0, id0, k, o, p, _before(o, p, wk, wi))


def _insert(key, ids, k: int, ck, ci, do) -> None:
    """``topk_insert`` on the rows ``do``: one compare-exchange per slot."""
    ck, ci = np.array(ck, dtype=_f32), np.array(ci, dtype=np.int64)
    for j in range(k):
        sw = do & _before(ck, ci, key[:, j], ids[:, j])
        tk, ti = key[:, j].copy(), ids[:, j].copy()
        key[:, j] = np.where(sw, ck, tk)
        ids[:, j] = np.where(sw, ci, ti)
        ck = np.where(sw, tk, ck)
        ci = np.where(sw, ti, ci)


def _compare(T: EntityTables, f: int, d):
    cf = int(T.cfun[f])
    d = np.asarray(d, dtype=_f32)
    if cf == CF_GAUSS:
        s = T.scales[f]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return np.exp((_f32(-0.69314718056) * d * d / (s * s)).astype(_f32)).astype(_f32)
    if cf == CF_DELTA:
        return (d != 0).astype(_f32)
    if cf == CF_EQUAL:
        return (d == 0).astype(_f32)
    return np.abs(d)


def _raw(T: EntityTables, feat: np.ndarray, i: int, metric: int) -> np.ndarray:
    """``raw_distance`` of entity ``i`` over the staged rows ``feat [n, F]``."""
    s = np.zeros(len(feat), dtype=_f32)
    c = T.ent[i]
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(T.n_feat):
            x = feat[:, f]
            miss = x != x
            v = _compare(T, f, (x - c[f]).astype(_f32))
            w = T.weights[f]
            if metric in (M_SQEUCLID, M_EUCLID):
                t = _fma((w * v).astype(_f32), v, s)
            elif metric == M_CITY:
                t = _fma(w, v, s)
            elif metric == M_CHEBY:
                t = np.maximum(s, (w * v).astype(_f32))
            else:
                t = _fma(w, np.power(v, _f32(T.p)).astype(_f32), s)
            s = np.where(miss, s, t).astype(_f32)
    return s


def _adjust(T: EntityTables, feat: np.ndarray):
    """``row_adjust``: ``(Σq / Σq_present or NaN, Σq_present)``, summed in field order in fp32."""
    qsum = _f32(0)
    qpresent = np.zeros(len(feat), dtype=_f32)
    for f in range(T.n_feat):
        q = T.qweights[f]
        qsum = _f32(qsum + q)
        qpresent = np.where(feat[:, f] == feat[:, f], (qpresent + q).astype(_f32), qpresent)
    with np.errstate(invalid="ignore", divide="ignore"):
        adj = np.where(qpresent > 0, (qsum / qpresent).astype(_f32), _f32(np.nan)).astype(_f32)
    return adj, qpresent


def _exact_rows(T: EntityTables, feat: np.ndarray, tile: np.ndarray, metric: int, K: int):
    """``exact_row`` over the staged rows: ``(key, ids, adj, present)``; named columns into ``tile``."""
    n = len(feat)
    adj, qpresent = _adjust(T, feat)
    key = np.full((n, K), np.inf, dtype=_f32)
    ids = np.full((n, K), _EMPTY_ID, dtype=np.int64)
    worst = np.full(n, np.inf, dtype=_f32)
    for i in range(T.n_ent):
        s = _raw(T, feat, i, metric)
        nc = _named_column(T, i)
        fin = s
        if not T.knn or nc >= 0:
            fin = _finish(T, s, adj)
        if nc >= 0:
            tile[:, nc] = fin
        ck = s if T.knn else fin
        ck = (-ck).astype(_f32) if T.similarity else ck
        do = _offer(ck, worst)
        _insert(key, ids, T.k, ck, np.full(n, i), do)
        worst = key[:, :T.k].max(axis=1)
    return key, ids, adj, qpresent > 0


def _mfma_rows(T: EntityTables, feat: np.ndarray, tile: np.ndarray, K: int):
    """The expansion over the staged rows without a missing value: ``(key, ids)``."""
    n, F = feat.shape
    Np, Fp = T.wc.shape
    xx = np.zeros(n, dtype=_f32)
    for f in range(F):
        xx = _fma((T.weights[f] * feat[:, f]).astype(_f32), feat[:, f], xx)
    lists = [(np.full((n, K), np.inf, dtype=_f32), np.full((n, K), _EMPTY_ID, dtype=np.int64)) for _ in range(2)]
    worst = [np.full(n, np.inf, dtype=_f32) for _ in range(2)]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(Np):
            acc = np.zeros(n, dtype=_f32)
            for f in range(F):
                acc = _fma(T.wc[i, f], feat[:, f], acc)
            d = (_fma(_f32(-2), acc, xx) + T.cc[i]).astype(_f32)
            if T.knn:
                d = np.maximum(d, _f32(0))
            nc = _named_column(T, i) if i < T.n_ent else -1
            if nc >= 0:
                tile[:, nc] = _finish(T, np.maximum(d, _f32(0)), _f32(1))
            h = (i >> 2) & 1  # the half-wave that holds entity i of its 32-entity tile
            key, ids = lists[h]
            _insert(key, ids, T.k, d, np.full(n, i), _offer(d, worst[h]))
            worst[h] = key[:, :T.k].max(axis=1)
    (key0, id0), (key1, id1) = lists
    _merge(key0, id0, key1, id1, T.k)
    return key0, id0


def _write_columns(T: EntityTables, key, ids, adj, finished: bool, clamp: bool, ok, tile) -> None:
    """``write_columns``: the ranked columns and the validity of the named ones."""
    n = len(key)

    def affinity(kv):
        v = (-kv).astype(_f32) if T.similarity else kv
        if clamp:
            v = np.maximum(v, _f32(0))
        return v if finished else _finish(T, v, adj)

    live = np.stack([np.isfinite(affinity(key[:, j])) for j in range(key.shape[1])], axis=1) \
        & (ids >= 0) & (ids < T.n_ent)
    ok = ok & (live[:, :T.k].all(axis=1) if T.knn else live[:, 0])
    nan = _f32(np.nan)
    for c, (op, arg, off, _) in enumerate(T.cols):
        if op == ENT_NAMED:
            src = _named_column(T, int(arg))
            tile[:, c] = np.where(ok, tile[:, src], nan) if 0 <= src <= c else nan
            continue
        r = _rank(int(arg))
        if not 0 <= r < T.k:
            tile[:, c] = nan
            continue
        v = affinity(key[:, r])
        ki = ids[:, r]
        got = ok & (ki >= 0) & (ki < T.n_ent) & np.isfinite(v)
        if op == ENT_AFFINITY:
            tile[:, c] = np.where(got, v, nan)
        else:
            tile[:, c] = np.where(got, T.tables[off + np.where(got, ki, 0)], nan)


def entities_numpy(X: np.ndarray, out: np.ndarray, tables: EntityTables, prep: Optional[np.ndarray] = None,
                   rows: Optional[int] = None) -> np.ndarray:
    """The kernel on the host, tile by tile: writes the columns ``tables.cols`` names into ``out``
    (fp32 ``[m, width]``, in place) and returns it."""
    T = tables
    X = np.asarray(X, dtype=np.float32)
    m = int(X.shape[0])
    if X.ndim != 2 or X.shape[1] != T.n_feat or out.shape != (m, T.width) or out.dtype != np.float32:
        raise ValueError(f"entities_numpy needs X [m, {T.n_feat}] and a float32 out [m, {T.width}]")
    TB = T.rows if rows is None else int(rows)
    K = template_k(T.k)
    for r0 in range(0, m, TB):
        r1 = min(m, r0 + TB)
        n = r1 - r0
        feat = X[r0:r1].copy()
        bad = np.zeros(n, dtype=bool)
        if prep is not None:
            for f in range(T.n_feat):
                bad |= prep_bad_numpy(X[r0:r1, f], prep, f)
                feat[:, f] = prep_numpy(X[r0:r1, f], prep, f)
        tile = np.full((n, len(T.cols)), np.nan, dtype=_f32)
        if T.wc is None:
            key, ids, adj, present = _exact_rows(T, feat, tile, T.metric, K)
            _write_columns(T, key, ids, adj, not T.knn, False, present & ~bad, tile)
        else:
            miss = np.isnan(feat).any(axis=1)
            for sel, exact in ((np.flatnonzero(~miss), False), (np.flatnonzero(miss), True)):
                if not len(sel):
                    continue
                sub = tile[sel]
                if exact:  # a row with a missing value: the VALU form over squared sums
                    key, ids, adj, present = _exact_rows(T, feat[sel], sub, M_SQEUCLID, K)
                    _write_columns(T, key, ids, adj, not T.knn, False, present & ~bad[sel], sub)
                else:
                    key, ids = _mfma_rows(T, feat[sel], sub, K)
                    _write_columns(T, key, ids, np.ones(len(sel), dtype=_f32), False, True, ~bad[sel], sub)
                tile[sel] = sub
        out[r0:r1, T.cols[:, 3]] = tile
    return out


__all__ = ["ENT_AFFINITY", "ENT_ID", "ENT_NAMED", "EntityTables", "LDS_BYTES", "MAX_COLUMNS", "MAX_FEATURES",
           "MAX_RANK", "ROWS", "entities_launch", "entities_numpy", "geometry", "lds_bytes", "prep_bad_numpy",
           "template_k"]
