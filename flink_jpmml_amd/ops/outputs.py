"""PMML ``<Output>`` columns of a scored batch on the device (``csrc/outputs.hip``) and its numpy twin.

``outputs_launch`` launches ``pmml_outputs_launch``: the raw results of a model plan in index mode
(``score`` = regression value or class / cluster index, ``valid``, optional ``probs [m, C]`` and
``affinity``) become the ``n_col`` columns of a column program, plus the reference score (the label
parsed as a double through ``label_table``).

A column program is ``int32 [n_col, 4]`` rows ``{op, arg, table_off, 0}``:

========================  ==========================================================================
``VALUE``                 the value where the row is valid, else NaN
``TABLE`` (``arg`` = L)   ``tables[table_off + idx]``; rows without an index read entry ``L`` (NaN)
``PROB`` (``arg`` = c)    ``probs[row, c]`` where valid
``PROB_WINNER``           ``probs[row, idx]`` where valid
``AFFINITY``              ``affinity[row]`` where valid
``CONST``                 ``tables[table_off]`` on every row
``NAN``                   NaN
``TOPK_INDEX`` / ``TOPK_PROB`` (``arg`` = rank r < k)
                          class / probability of the r-th largest probability: ties to the lower
                          class, a NaN is never selected, NaN past the non-NaN classes and on
                          invalid rows
========================  ==========================================================================

``outputs_numpy`` walks the same tiles with the same clamps and the same tie rule on the host.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

OP_VALUE, OP_TABLE, OP_PROB, OP_PROB_WINNER, OP_AFFINITY, OP_CONST, OP_NAN, OP_TOPK_INDEX, OP_TOPK_PROB = range(9)

TILE_BYTES = 64 * 1024  # both LDS tiles of one workgroup: two workgroups fit a CU's 160 KiB
MAX_CLASSES = 256  # SEG_MAXC
MAX_COLUMNS = 64
MAX_TOP_K = 8
THREADS = 256


def rows_per_block(C: int, n_col: int) -> int:
    """``R``: consecutive rows one workgroup owns (``outputs.hip`` ``out_rows``): the ``R x C``
    probabilities and the ``R x n_col`` outputs, each with an odd row stride, in ``TILE_BYTES``."""
    if not 0 <= C <= MAX_CLASSES or not 1 <= n_col <= MAX_COLUMNS:
        raise ValueError(f"outputs kernel handles 0 <= C <= {MAX_CLASSES} and 1 <= n_col <= {MAX_COLUMNS}, "
                         f"got C={C}, n_col={n_col}")
    words = ((C | 1) if C > 0 else 0) + (n_col | 1)
    return max(1, min(THREADS, TILE_BYTES // (4 * words)))


def _check(m: int, C: int, n_col: int, k: int, prog_rows: int) -> None:
    rows_per_block(C, n_col)
    if not 0 <= k <= MAX_TOP_K:
        raise ValueError(f"top_k must be in [0, {MAX_TOP_K}], got {k}")
    if prog_rows != n_col:
        raise ValueError(f"column program has {prog_rows} rows for {n_col} columns")
    if m < 0:
        raise ValueError("negative row count")


def outputs_launch(score, valid, out, prog, tables, probs=None, affinity=None, label_table=None, k: int = 0,
                   score_out=None, valid_out=None, stream=None) -> None:
    """Device tensors: ``score`` fp32 ``[m]``, ``valid`` uint8 ``[m]``, ``out`` fp32 ``[m, n_col]``
    (unit column stride, any row stride), ``prog`` int32 ``[n_col, 4]``, ``tables`` fp32 pool,
    ``probs`` fp32 ``[m, C]`` (unit column stride) or None, ``affinity`` fp32 ``[m]`` or None,
    ``label_table`` fp32 ``[L + 1]`` (last NaN) or None, ``score_out`` / ``valid_out`` or None."""
    from . import _lib

    m, n_col = int(out.shape[0]), int(out.shape[1])
    C = int(probs.shape[1]) if probs is not None else 0
    _check(m, C, n_col, int(k), int(prog.shape[0]))
    if int(score.numel()) < m or int(valid.numel()) < m or not score.is_contiguous() or not valid.is_contiguous():
        raise ValueError("outputs_launch needs contiguous score / valid of m rows")
    if out.stride(1) != 1 or (m > 1 and out.stride(0) < n_col):
        raise ValueError("outputs_launch needs a row-major out with unit column stride")
    if probs is not None and (int(probs.shape[0]) < m or (C > 1 and probs.stride(1) != 1)
                              or (m > 1 and probs.stride(0) < C)):
        raise ValueError("outputs_launch needs row-major probs of m rows with unit column stride")
    if affinity is not None and (int(affinity.numel()) < m or not affinity.is_contiguous()):
        raise ValueError("outputs_launch needs a contiguous affinity of m rows")
    if not prog.is_contiguous() or int(prog.shape[1]) != 4 or not tables.is_contiguous():
        raise ValueError("outputs_launch needs a contiguous [n_col, 4] program and a contiguous table pool")
    for o in (score_out, valid_out):
        if o is not None and (int(o.numel()) < m or not o.is_contiguous()):
            raise ValueError("outputs_launch needs contiguous score_out / valid_out of m rows")
    if (score_out is None) != (valid_out is None):
        raise ValueError("score_out and valid_out go together")
    a = _lib.OutputArgs()
    a.score, a.valid, a.out = score.data_ptr(), valid.data_ptr(), out.data_ptr()
    a.probs = probs.data_ptr() if probs is not None and C > 0 else None
    a.affinity = affinity.data_ptr() if affinity is not None else None
    a.prog, a.tables = prog.data_ptr(), tables.data_ptr()
    a.label_table = label_table.data_ptr() if label_table is not None else None
    a.n_labels = int(label_table.numel()) - 1 if label_table is not None else 0
    a.score_out = score_out.data_ptr() if score_out is not None else None
    a.valid_out = valid_out.data_ptr() if valid_out is not None else None
    a.m, a.C, a.n_col, a.k, a.n_tables = m, C, n_col, int(k), int(tables.numel())
    a.ldp = int(probs.stride(0)) if probs is not None and m > 1 else C
    a.ldo = int(out.stride(0)) if m > 1 else n_col
    _lib.check(_lib.load().pmml_outputs_launch(_lib.stream_handle(stream), a), "pmml_outputs_launch")


def _index(s: np.ndarray, okidx: np.ndarray, n: int, other: int) -> np.ndarray:
    """The kernel's index of a row: ``int(s)`` where the row has one in ``[0, n)``, else ``other``."""
    with np.errstate(invalid="ignore"):
        good = okidx & (s >= 0) & (s < np.float32(n))
    return np.where(good, np.where(good, s, 0).astype(np.int64), other)


def _top_k(P: np.ndarray, ok: np.ndarray, K: int):
    """The kernel's register chain over a tile: scan the classes in order, an offered value takes
    the first slot that is empty or holds a strictly smaller value, what it displaces moves down."""
    n, C = P.shape
    v = np.full((n, max(K, 1)), np.nan, dtype=np.float32)
    idx = np.full((n, max(K, 1)), -1, dtype=np.int64)
    for c in range(C if K else 0):
        p = P[:, c].copy()
        ci = np.full(n, c, dtype=np.int64)
        offer = ok & (p == p)  # invalid rows and NaN offer nothing
        taken = np.zeros(n, dtype=bool)
        for j in range(K):
            with np.errstate(invalid="ignore"):
                take = offer & (taken | (idx[:, j] < 0) | (p > v[:, j]))
            tv, ti = v[:, j].copy(), idx[:, j].copy()
            v[:, j] = np.where(take, p, tv)
            idx[:, j] = np.where(take, ci, ti)
            p = np.where(take, tv, p)
            ci = np.where(take, ti, ci)
            taken |= take
    return v, idx


def outputs_numpy(score: np.ndarray, valid: np.ndarray, prog: np.ndarray, tables: np.ndarray,
                  probs: Optional[np.ndarray] = None, affinity: Optional[np.ndarray] = None,
                  label_table: Optional[np.ndarray] = None, k: int = 0):
    """The kernel on the host, tile by tile. Returns ``(out float32 [m, n_col], score_out float32
    [m], valid_out uint8 [m])``."""
    score = np.asarray(score, dtype=np.float32)
    valid = np.asarray(valid)
    prog = np.asarray(prog, dtype=np.int32).reshape(-1, 4)
    tables = np.asarray(tables, dtype=np.float32).reshape(-1)
    m, n_col = int(score.shape[0]), int(prog.shape[0])
    C = int(probs.shape[1]) if probs is not None else 0
    _check(m, C, n_col, int(k), n_col)
    if C == 0:
        probs, k = None, 0
    K = next(x for x in (0, 1, 2, 4, 8) if x >= k)
    nan = np.float32(np.nan)
    n_tab = int(tables.size)
    out = np.empty((m, n_col), dtype=np.float32)
    score_out = np.empty(m, dtype=np.float32)
    valid_out = np.empty(m, dtype=np.uint8)
    R = rows_per_block(C, n_col)
    for r0 in range(0, m, R):
        r1 = min(m, r0 + R)
        n = r1 - r0
        s = score[r0:r1]
        ok = valid[r0:r1] != 0
        okidx = ok & (s == s)
        P = np.asarray(probs[r0:r1], dtype=np.float32) if probs is not None else np.empty((n, 0), np.float32)
        tv, ti = _top_k(P, ok, K)
        rows = np.arange(n)
        for j in range(n_col):
            op, arg, off = int(prog[j, 0]), int(prog[j, 1]), int(prog[j, 2])
            x = np.full(n, nan, dtype=np.float32)
            if op == OP_VALUE:
                x = np.where(ok, s, nan)
            elif op == OP_TABLE:
                if arg >= 0 and off >= 0:
                    pos = off + _index(s, okidx, arg, arg)
                    inside = pos < n_tab
                    x = np.where(inside, tables[np.where(inside, pos, 0)] if n_tab else nan, nan)
            elif op == OP_PROB:
                if 0 <= arg < C:
                    x = np.where(ok, P[:, arg], nan)
            elif op == OP_PROB_WINNER:
                if C > 0:
                    x = np.where(ok, P[rows, _index(s, okidx, C, 0)], nan)
            elif op == OP_AFFINITY:
                if affinity is not None:
                    x = np.where(ok, np.asarray(affinity[r0:r1], dtype=np.float32), nan)
            elif op == OP_CONST:
                if 0 <= off < n_tab:
                    x = np.full(n, tables[off], dtype=np.float32)
            elif op in (OP_TOPK_INDEX, OP_TOPK_PROB):
                if 0 <= arg < k and arg < K:
                    if op == OP_TOPK_PROB:
                        x = tv[:, arg]
                    else:
                        x = np.where(ti[:, arg] >= 0, ti[:, arg].astype(np.float32), nan)
            out[r0:r1, j] = x.astype(np.float32)
        if label_table is not None:
            lt = np.asarray(label_table, dtype=np.float32).reshape(-1)
            L = int(lt.size) - 1
            so = lt[_index(s, okidx, L, L)]
            vo = ok & (so == so)
            score_out[r0:r1] = np.where(vo, so, nan)
            valid_out[r0:r1] = vo
        else:
            score_out[r0:r1] = s
            valid_out[r0:r1] = ok
    return out, score_out, valid_out


__all__ = ["MAX_CLASSES", "MAX_COLUMNS", "MAX_TOP_K", "OP_AFFINITY", "OP_CONST", "OP_NAN", "OP_PROB",
           "OP_PROB_WINNER", "OP_TABLE", "OP_TOPK_INDEX", "OP_TOPK_PROB", "OP_VALUE", "outputs_launch",
           "outputs_numpy", "rows_per_block"]
