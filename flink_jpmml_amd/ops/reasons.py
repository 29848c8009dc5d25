"""Scorecard reason codes of a scored batch on the device (``csrc/reasons.hip``) and its numpy twin.

``reasons_launch`` launches ``pmml_reasons_launch`` over the matrix the scorecard's general tree
kernel scored (raw rows plus the ``FieldPrep`` table, or the prepared tile of a derive pass) and the
``valid`` bytes the score plan wrote. A :class:`ReasonTables` holds the packed scorecard:

==============  ==============================================================================
``chars``       ``int32 [n_char, 2]`` ``{first attribute, attribute count}``, document order
``attrs``       ``int32 [n_attr, 4]`` ``{predicate offset, code index or -1, value column or -1, 0}``
``dval``        ``float64 [n_attr]``: the point difference ``d`` of a constant partial score, or the
                baseline of an attribute whose partial score is a column (``ComplexPartialScore``)
``preds``       ``int32 [n, 4]`` postfix predicate programs, ``pool`` their set values
                (``runtime/general_tree.py::_PredCompiler``)
``cols``        ``int32 [n_col, 4]`` ``{rank (0-based), table offset, destination column, 0}``
``tables``      ``float32``: per column the encodings of the ``n_code`` codes
==============  ==============================================================================

Per row: the first TRUE attribute of each characteristic (UNKNOWN does not match), its difference in
float64 (``base - x`` or, with ``above``, ``x - base`` for a value column), summed per code in
characteristic order; the codes ranked by descending sum, ties to the code touched first on the row.
``shared`` selects the accumulator path (a code belongs to several characteristics); without it every
sum has one addend and the top K are a compare-insert chain, strict ``>``.

``reasons_numpy`` walks the same tiles with the same rules on the host.
"""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

P_END, P_TRUE, P_FALSE, P_GE, P_EQ, P_ISMISS, P_NOTMISS, P_SET, P_AND, P_OR, P_XOR, P_SURR = range(12)
V_F, V_T, V_U = 0, 1, 2

MAX_RANK = 8
MAX_CODES = 64
MAX_COLUMNS = 64
LDS_BYTES = 64 * 1024  # one workgroup's request: two workgroups share a CU's 160 KiB
ROWS = (256, 128, 64)  # rows (= lanes) of one workgroup, the first that fits

# FieldPrep.flags (csrc/common.h)
FP_HAS_MISSING_REPL, FP_HAS_INTERVAL, FP_LO_OPEN, FP_HI_OPEN = 1 << 0, 1 << 1, 1 << 2, 1 << 3
FP_INVALID_RETURN, FP_INVALID_AS_MISSING, FP_INVALID_AS_VALUE = 1 << 4, 1 << 5, 1 << 6
FP_OUTLIER_AS_MISSING, FP_OUTLIER_AS_EXTREME, FP_INTEGER, FP_CODE_RANGE = 1 << 7, 1 << 8, 1 << 9, 1 << 10
FP_ROW_INVALID, FP_MISSING_VALUE, FP_VALUE_MASK, FP_VALUE_LIST = 1 << 11, 1 << 12, 1 << 13, 1 << 14


def template_k(k: int) -> int:
    """The kernel instantiation (1, 2, 4, 8) that serves ranks ``1 .. k``."""
    if not 1 <= k <= MAX_RANK:
        raise ValueError(f"reason code rank must be in [1, {MAX_RANK}], got {k}")
    return next(x for x in (1, 2, 4, 8) if x >= k)


def lds_bytes(n_feat: int, n_code: int, rows: int, shared: bool, feat_lds: bool) -> int:
    """LDS request of one workgroup (``reasons.hip`` ``rc_lds_bytes``): the ``[F][rows]`` fp32
    feature planes plus, on the shared path, ``[R][rows]`` float64 sums and int32 touch numbers."""
    return (n_feat * rows * 4 if feat_lds else 0) + (n_code * rows * 12 if shared else 0)


def geometry(n_feat: int, n_code: int, shared: bool) -> Tuple[int, bool]:
    """``(rows, feat_lds)``: 256, 128 or 64 rows per workgroup with the features staged in LDS when
    that fits ``LDS_BYTES``, else the features read from global memory. ``ValueError`` when even 64
    rows of accumulators do not fit."""
    for feat_lds in (True, False):
        for rows in ROWS:
            if lds_bytes(n_feat, n_code, rows, shared, feat_lds) <= LDS_BYTES:
                return rows, feat_lds
    raise ValueError(f"{n_code} reason codes need {lds_bytes(n_feat, n_code, 64, shared, False)} bytes of LDS "
                     f"for 64 rows > {LDS_BYTES}")


class ReasonTables:
    """The packed scorecard (module docstring), checked once: every index a lane follows stays
    inside its table, every predicate program ends, every destination column is inside the matrix."""

    def __init__(self, chars, attrs, dval, preds, pool, cols, tables, n_code: int, n_feat: int, width: int,
                 above: bool, shared: bool):
        self.chars = np.ascontiguousarray(chars, dtype=np.int32).reshape(-1, 2)
        self.attrs = np.ascontiguousarray(attrs, dtype=np.int32).reshape(-1, 4)
        self.dval = np.ascontiguousarray(dval, dtype=np.float64).reshape(-1)
        self.preds = np.ascontiguousarray(preds, dtype=np.int32).reshape(-1, 4)
        self.pool = np.ascontiguousarray(pool, dtype=np.float32).reshape(-1)
        self.cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1, 4)
        self.tables = np.ascontiguousarray(tables, dtype=np.float32).reshape(-1)
        self.n_code, self.n_feat, self.width = int(n_code), int(n_feat), int(width)
        self.above, self.shared = bool(above), bool(shared)
        self.k = int(self.cols[:, 0].max()) + 1 if len(self.cols) else 0
        self._check()
        self._device = {}

    def _check(self) -> None:
        n_attr, n_pred = len(self.attrs), len(self.preds)
        if not 1 <= self.n_code <= MAX_CODES:
            raise ValueError(f"reason kernel handles 1 .. {MAX_CODES} codes, got {self.n_code}")
        if not 1 <= len(self.cols) <= MAX_COLUMNS or not 1 <= self.k <= MAX_RANK or (self.cols[:, 0] < 0).any():
            raise ValueError(f"reason kernel handles 1 .. {MAX_COLUMNS} columns of rank 1 .. {MAX_RANK}")
        if self.n_feat < 1 or self.width < 1 or len(self.dval) != n_attr or self.pool.size < 1:
            raise ValueError("reason tables: empty matrix, pool or mismatched attribute tables")
        if ((self.chars < 0).any() or (self.chars.sum(axis=1) > n_attr).any()):
            raise ValueError("reason tables: a characteristic's attributes lie outside the attribute table")
        at = self.attrs
        if ((at[:, 0] < 0) | (at[:, 0] >= n_pred)).any() or (at[:, 1] >= self.n_code).any() \
                or (at[:, 2] >= self.n_feat).any():
            raise ValueError("reason tables: an attribute points outside its tables")
        if n_pred == 0 or (self.preds[-1, 0] & 0xFF) != P_END:
            raise ValueError("reason tables: the last predicate program does not end")
        for op, f, a, cnt in self.preds:
            op &= 0xFF
            if op > P_SURR:
                raise ValueError(f"reason tables: predicate op {op}")
            if op in (P_GE, P_EQ, P_ISMISS, P_NOTMISS, P_SET) and not 0 <= f < self.n_feat:
                raise ValueError("reason tables: a predicate reads a column outside the matrix")
            if op == P_SET and not (0 <= a and 0 <= cnt and a + cnt <= self.pool.size):
                raise ValueError("reason tables: a set predicate reads outside the pool")
        c = self.cols
        if ((c[:, 1] < 0) | (c[:, 1] + self.n_code > self.tables.size)).any() \
                or ((c[:, 2] < 0) | (c[:, 2] >= self.width)).any():
            raise ValueError("reason tables: a column's table or destination is out of range")

    def on(self, device):
        """The tables as device tensors (cached per device)."""
        import torch

        key = str(device)
        d = self._device.get(key)
        if d is None:
            d = self._device[key] = {k: torch.from_numpy(getattr(self, k)).to(device)
                                     for k in ("chars", "attrs", "dval", "preds", "pool", "cols", "tables")}
        return d


def reasons_launch(X, valid, out, tables: ReasonTables, prep=None, rows: Optional[int] = None,
                   feat_lds: Optional[bool] = None, stream=None) -> None:
    """Device tensors: ``X`` fp32 ``[m, n_feat]`` (unit column stride, any row stride), ``valid``
    uint8 ``[m]``, ``out`` fp32 ``[m, width]`` (unit column stride, any row stride): only the
    columns ``tables.cols`` names are written. ``prep``: the int32 ``FieldPrep`` table of raw rows,
    None for a prepared tile. ``rows`` / ``feat_lds`` override :func:`geometry`."""
    from . import _lib

    T = tables
    m = int(X.shape[0])
    if X.dim() != 2 or int(X.shape[1]) != T.n_feat or (T.n_feat > 1 and X.stride(1) != 1) \
            or (m > 1 and X.stride(0) < T.n_feat):
        raise ValueError(f"reasons_launch needs a row-major [m, {T.n_feat}] X with unit column stride")
    if out.dim() != 2 or int(out.shape[0]) != m or int(out.shape[1]) != T.width \
            or (T.width > 1 and out.stride(1) != 1) or (m > 1 and out.stride(0) < T.width):
        raise ValueError(f"reasons_launch needs a row-major [m, {T.width}] out with unit column stride")
    if int(valid.numel()) < m or not valid.is_contiguous():
        raise ValueError("reasons_launch needs a contiguous valid of m rows")
    if prep is not None and (not prep.is_contiguous() or int(prep.numel()) < 8 * T.n_feat):
        raise ValueError("reasons_launch needs a contiguous FieldPrep table of n_feat records")
    g_rows, g_lds = geometry(T.n_feat, T.n_code, T.shared)
    rows = g_rows if rows is None else int(rows)
    feat_lds = g_lds if feat_lds is None else bool(feat_lds)
    if rows not in ROWS or lds_bytes(T.n_feat, T.n_code, rows, T.shared, feat_lds) > LDS_BYTES:
        raise ValueError(f"reasons_launch: {rows} rows per workgroup do not fit {LDS_BYTES} bytes of LDS")
    d = T.on(X.device)
    a = _lib.ReasonArgs()
    a.X, a.prep, a.valid = X.data_ptr(), (prep.data_ptr() if prep is not None else None), valid.data_ptr()
    a.chars, a.attrs, a.dval = d["chars"].data_ptr(), d["attrs"].data_ptr(), d["dval"].data_ptr()
    a.preds, a.pool = d["preds"].data_ptr(), d["pool"].data_ptr()
    a.cols, a.tables, a.out = d["cols"].data_ptr(), d["tables"].data_ptr(), out.data_ptr()
    a.n_rows, a.n_feat = m, T.n_feat
    a.ldx = int(X.stride(0)) if m > 1 else T.n_feat
    a.ldo = int(out.stride(0)) if m > 1 else T.width
    a.n_char, a.n_code, a.n_col, a.k = len(T.chars), T.n_code, len(T.cols), T.k
    a.above, a.shared, a.feat_lds, a.rows = int(T.above), int(T.shared), int(feat_lds), rows
    a.n_tables = int(T.tables.size)
    _lib.check(_lib.load().pmml_reasons_launch(_lib.stream_handle(stream), a), "pmml_reasons_launch")


# --------------------------------------------------------------------------- numpy twin


def prep_numpy(x: np.ndarray, prep: np.ndarray, f: int) -> np.ndarray:
    """``common.h::prep_value`` of column ``f`` over fp32 values ``x`` (``prep``: the raw uint32
    ``[F (+ lists), 8]`` table of ``build_field_prep``). The row-rejected flag is not returned: the
    score plan's ``valid`` already carries it."""
    x = np.asarray(x, dtype=np.float32).copy()
    raw = np.asarray(prep).view(np.uint32).reshape(-1, 8)
    rec = raw[f]
    fl = int(rec[0])
    if fl == 0 or fl & FP_ROW_INVALID:
        return x
    lo, hi, mrepl, irepl, out_lo, out_hi, pad = (np.float32(v) for v in rec[1:8].view(np.float32))
    nan = np.float32(np.nan)
    with np.errstate(invalid="ignore"):
        miss = x != x
        if fl & FP_MISSING_VALUE:
            miss |= x == pad
        vlist, n_miss, n_inv = None, 0, 0
        if fl & FP_VALUE_LIST:
            w = int(rec[7])
            vlist = raw.reshape(-1).view(np.float32)[8 * f + (w & 0xFFFF):]
            n_miss, n_inv = (w >> 16) & 0xFF, w >> 24
            for i in range(n_miss):
                miss |= x == vlist[i]
        invalid = np.zeros(len(x), dtype=bool)
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
            k = np.where(inside, d, 0).astype(np.int64)
            bits = (int(rec[5]) | (int(rec[6]) << 32))
            inside &= np.array([(bits >> int(v)) & 1 for v in k], dtype=bool)
            invalid |= ~inside
        invalid &= ~miss
        valid = ~miss & ~invalid
        if fl & FP_INVALID_AS_MISSING and not fl & FP_INVALID_RETURN:
            miss |= invalid
        elif fl & FP_INVALID_AS_VALUE and not fl & FP_INVALID_RETURN:
            x = np.where(invalid, irepl, x)
        if fl & FP_OUTLIER_AS_MISSING:
            miss = np.where(valid, (x < out_lo) | (x > out_hi), miss)
        elif fl & FP_OUTLIER_AS_EXTREME:
            x = np.where(valid, np.minimum(np.maximum(x, out_lo), out_hi), x)
    return np.where(miss, mrepl if fl & FP_HAS_MISSING_REPL else nan, x).astype(np.float32)


# The rules the tests' mutants replace one at a time.
_ACC = np.float64  # differences and their sums


def _match(v: np.ndarray) -> np.ndarray:
    """An attribute is taken when its predicate is TRUE; UNKNOWN does not match."""
    return v == V_T


def _beats(p: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Strict: an equal value never displaces an earlier one."""
    with np.errstate(invalid="ignore"):
        return p > v


def _tie(t: np.ndarray, bt: np.ndarray) -> np.ndarray:
    """Equal sums: the code touched first on the row wins."""
    return t < bt


def _eval(T: ReasonTables, pc: int, feature, n: int) -> np.ndarray:
    """``reasons.hip::rc_eval`` over a tile: the value (0 / 1 / 2) of the program at ``pc`` per row."""
    preds, pool = T.preds, T.pool
    thr = preds[:, 3].copy().view(np.float32)
    st = []
    while True:
        op, f, a, cnt = (int(v) for v in preds[pc])
        neg, op = (op >> 8) & 1, op & 0xFF
        if op == P_END:
            return st[-1] if st else np.zeros(n, dtype=np.uint8)
        if op >= P_AND:
            vals = st[len(st) - f:]
            del st[len(st) - f:]
            E = np.stack(vals) if vals else np.zeros((0, n), dtype=np.uint8)
            any_t, any_f, any_u = (E == V_T).any(axis=0), (E == V_F).any(axis=0), (E == V_U).any(axis=0)
            if op == P_AND:
                v = np.where(any_f, V_F, np.where(any_u, V_U, V_T))
            elif op == P_OR:
                v = np.where(any_t, V_T, np.where(any_u, V_U, V_F))
            elif op == P_XOR:
                v = np.where(any_u, V_U, (E == V_T).sum(axis=0) % 2)
            else:  # surrogate: the first known value, UNKNOWN when there is none
                v = np.full(n, V_U)
                for e in reversed(vals):
                    v = np.where(e != V_U, e, v)
        elif op == P_TRUE:
            v = np.full(n, V_T)
        elif op == P_FALSE:
            v = np.full(n, V_F)
        else:
            x = feature(f)
            miss = x != x
            if op == P_ISMISS:
                v = np.where(miss, V_T, V_F)
            elif op == P_NOTMISS:
                v = np.where(miss, V_F, V_T)
            else:
                with np.errstate(invalid="ignore"):
                    if op == P_GE:
                        r = x >= thr[pc]
                    elif op == P_EQ:
                        r = x == thr[pc]
                    else:
                        r = np.zeros(n, dtype=bool)
                        for i in range(cnt):
                            r |= pool[a + i] == x
                v = np.where(miss, V_U, r.astype(np.int64) ^ neg)
        st.append(np.asarray(v, dtype=np.uint8))
        pc += 1


def reasons_numpy(X: np.ndarray, valid: np.ndarray, out: np.ndarray, tables: ReasonTables,
                  prep: Optional[np.ndarray] = None, rows: Optional[int] = None) -> np.ndarray:
    """The kernel on the host, tile by tile: writes the columns ``tables.cols`` names into ``out``
    (fp32 ``[m, width]``, in place) and returns it."""
    T = tables
    X = np.asarray(X, dtype=np.float32)
    valid = np.asarray(valid)
    m = int(X.shape[0])
    if X.ndim != 2 or X.shape[1] != T.n_feat or out.shape != (m, T.width) or out.dtype != np.float32:
        raise ValueError(f"reasons_numpy needs X [m, {T.n_feat}] and a float32 out [m, {T.width}]")
    TB = geometry(T.n_feat, T.n_code, T.shared)[0] if rows is None else int(rows)
    K = template_k(T.k)
    nan = np.float32(np.nan)
    for r0 in range(0, m, TB):
        r1 = min(m, r0 + TB)
        n = r1 - r0
        staged = {}

        def feature(f: int, r0=r0, r1=r1, staged=staged) -> np.ndarray:
            x = staged.get(f)
            if x is None:
                x = X[r0:r1, f]
                x = staged[f] = prep_numpy(x, prep, f) if prep is not None else x
            return x

        ok = valid[r0:r1] != 0
        tv = np.zeros((n, K), dtype=_ACC)
        ti = np.full((n, K), -1, dtype=np.int64)
        acc = np.zeros((n, T.n_code), dtype=_ACC)
        touch = np.zeros((n, T.n_code), dtype=np.int64)
        n_touched = np.zeros(n, dtype=np.int64)
        lanes = np.arange(n)
        for a0, na in T.chars:
            pick = np.full(n, -1, dtype=np.int64)
            for j in range(a0, a0 + na):
                hit = _match(_eval(T, int(T.attrs[j, 0]), feature, n)) & (pick < 0)
                pick = np.where(hit, j, pick)
            code = np.where(pick >= 0, T.attrs[np.maximum(pick, 0), 1], -1)
            vcol = np.where(pick >= 0, T.attrs[np.maximum(pick, 0), 2], -1)
            d = T.dval[np.maximum(pick, 0)].astype(np.float64)
            for f in np.unique(vcol[vcol >= 0]):
                x = feature(int(f)).astype(np.float64)
                with np.errstate(invalid="ignore"):
                    d = np.where(vcol == f, (x - d) if T.above else (d - x), d)
            d = d.astype(_ACC)
            offer = ok & (code >= 0)
            c = np.where(offer, code, 0)
            if T.shared:
                with np.errstate(invalid="ignore"):
                    acc[lanes, c] = np.where(offer, acc[lanes, c] + d, acc[lanes, c])
                first = offer & (touch[lanes, c] == 0)
                n_touched = n_touched + first
                touch[lanes, c] = np.where(first, n_touched, touch[lanes, c])
                continue
            p, ci = d.copy(), code.copy()
            taken = np.zeros(n, dtype=bool)
            for j in range(K):  # the register chain: first slot that is empty or holds strictly less
                take = offer & (taken | (ti[:, j] < 0) | _beats(p, tv[:, j]))
                ov, oi = tv[:, j].copy(), ti[:, j].copy()
                tv[:, j] = np.where(take, p, ov)
                ti[:, j] = np.where(take, ci, oi)
                p = np.where(take, ov, p)
                ci = np.where(take, oi, ci)
                taken |= take
        if T.shared:
            for r in range(K):  # selection passes
                best = np.full(n, -1, dtype=np.int64)
                bv = np.zeros(n, dtype=_ACC)
                bt = np.zeros(n, dtype=np.int64)
                for c in range(T.n_code):
                    t, v = touch[:, c], acc[:, c]
                    with np.errstate(invalid="ignore"):
                        better = (t > 0) & ((best < 0) | _beats(v, bv) | ((v == bv) & _tie(t, bt)))
                    best = np.where(better, c, best)
                    bv = np.where(better, v, bv)
                    bt = np.where(better, t, bt)
                ti[:, r] = best
                sel = best >= 0
                touch[lanes[sel], best[sel]] = -1
        for r, off, dst, _ in T.cols:
            code = ti[:, r] if r < T.k else np.full(n, -1)
            got = ok & (code >= 0)
            out[r0:r1, dst] = np.where(got, T.tables[off + np.where(got, code, 0)], nan)
    return out


__all__ = ["LDS_BYTES", "MAX_CODES", "MAX_COLUMNS", "MAX_RANK", "ROWS", "ReasonTables", "geometry", "lds_bytes",
           "prep_numpy", "reasons_launch", "reasons_numpy", "template_k"]
