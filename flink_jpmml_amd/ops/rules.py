"""Ranked association rules of a batch of baskets on the device (``csrc/rules.hip``) and its numpy twin.

``rules_launch`` launches ``pmml_rules_launch`` over the raw ``[m, F]`` fp32 rows of an
AssociationModel and the document's ``FieldPrep`` table. A :class:`RuleTables` holds the packed model:

==============  ==============================================================================
``fields``      ``int32 [F, 4]`` ``{kind, imap offset, count, nvals offset}``: ``FIELD_CODES`` maps
                the vocabulary code ``int(x)`` of a string field through ``imap``, ``FIELD_VALUES``
                finds ``x`` in ``count`` sorted fp32 values of ``nvals`` and maps its position
``imap``        ``int32``: the item a code / a value names, ``-1`` for none
``nvals``       ``float32``: the sorted item values of the numeric fields
``sets``        ``int32 [n_set, 2]`` ``{first pair, pair count}``, an itemset word-sparse
``pairs``       ``uint32 [n_pair, 2]`` ``{basket word, mask of the itemset's items in it}``
``rules``       ``int32 [n_rules, 2]`` ``{antecedent set, consequent set}``, document order
``order``       ``int32 [n_group, n_rules]``: per scan group the rule indices sorted by the oracle's
                key (``sign * measure``, a missing measure as ``-inf``, document order on ties)
``scan``        ``int32 [n_group, n_rules, 4]``, derived from the four above: what the kernel walks,
                one record per step ``{rule index, first antecedent pair, first consequent pair,
                antecedent pairs | consequent pairs << 8}`` in ``order``
``groups``      ``int32 [n_group, 2]`` ``{algorithm, ranks the group's columns read}``
``cols``        ``int32 [n_col, 4]`` ``{group, rank (0-based), table offset, destination column}``
``tables``      ``float32``: per column the values of the ``n_rules`` rules and a NaN
==============  ==============================================================================

Per row: the basket is the set of items its prepared values name; per group the rules are walked in
``order`` and the first ``R`` matches kept (``recommendation``: antecedent inside the basket;
``exclusiveRecommendation``: and the whole consequent not inside; ``ruleAssociation``: both inside);
column ``j`` is ``tables[off_j + index of its (group, rank) match]``, NaN with fewer matches and on a
row the preparation rejects.

``rules_numpy`` walks the same tiles with the same statements on the host.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from .entities import prep_bad_numpy
from .reasons import prep_numpy

ALG_RECOMMENDATION, ALG_EXCLUSIVE, ALG_ASSOCIATION = range(3)
ALGORITHMS = {"recommendation": ALG_RECOMMENDATION, "exclusiveRecommendation": ALG_EXCLUSIVE,
              "ruleAssociation": ALG_ASSOCIATION}
FIELD_NONE, FIELD_CODES, FIELD_VALUES = range(3)

MAX_ITEMS = 1024
MAX_RULES = 4096
MAX_SET_ITEMS = 16
MAX_FIELDS = 128
MAX_RANK = 8
MAX_GROUPS = 4
MAX_COLUMNS = 64
REG_WORDS = 4  # baskets of up to 128 items live in registers
LDS_BYTES = 64 * 1024  # one workgroup's request: two workgroups share a CU's 160 KiB
ROWS = (256, 128, 64)  # rows (= lanes) of one workgroup, the first that fits


def template_r(k: int) -> int:
    """The kernel instantiation (1, 2, 4, 8) that serves ranks ``1 .. k``."""
    if not 1 <= k <= MAX_RANK:
        raise ValueError(f"rule rank must be in [1, {MAX_RANK}], got {k}")
    return next(x for x in (1, 2, 4, 8) if x >= k)


def words(n_items: int) -> int:
    return (n_items + 31) // 32


def lds_bytes(n_feat: int, n_items: int, rows: int) -> int:
    """LDS request of one workgroup (``rules.hip`` ``rl_lds_bytes``): the ``[F][rows]`` fp32 planes,
    the ``[rows]`` rejected flags and, past ``REG_WORDS`` words, the ``[W][rows]`` baskets."""
    W = words(n_items)
    return (n_feat + 1 + (W if W > REG_WORDS else 0)) * rows * 4


def geometry(n_feat: int, n_items: int) -> int:
    """Rows per workgroup: 256, 128 or 64, the first whose request fits ``LDS_BYTES``."""
    for rows in ROWS:
        if lds_bytes(n_feat, n_items, rows) <= LDS_BYTES:
            return rows
    raise ValueError(f"{n_feat} fields and {n_items} items need {lds_bytes(n_feat, n_items, 64)} bytes of LDS "
                     f"for 64 rows > {LDS_BYTES}")


class RuleTables:
    """The packed model (module docstring), checked once: every index a lane follows stays inside
    its table and every destination column inside the matrix."""

    _ARRAYS = ("fields", "imap", "nvals", "sets", "pairs", "rules", "order", "groups", "cols", "tables")
    _KERNEL = ("fields", "imap", "nvals", "pairs", "scan", "groups", "cols", "tables")  # what a launch reads

    def __init__(self, fields, imap, nvals, sets, pairs, rules, order, groups, cols, tables, n_items: int,
                 width: int):
        self.fields = np.ascontiguousarray(fields, dtype=np.int32).reshape(-1, 4)
        self.imap = np.ascontiguousarray(imap if len(imap) else [-1], dtype=np.int32).reshape(-1)
        self.nvals = np.ascontiguousarray(nvals if len(nvals) else [0.0], dtype=np.float32).reshape(-1)
        self.sets = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 2)
        self.pairs = np.ascontiguousarray(pairs if len(pairs) else [(0, 0)], dtype=np.uint32).reshape(-1, 2)
        self.rules = np.ascontiguousarray(rules, dtype=np.int32).reshape(-1, 2)
        self.groups = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1, 2)
        self.order = np.ascontiguousarray(order, dtype=np.int32).reshape(len(self.groups), -1)
        self.cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1, 4)
        self.tables = np.ascontiguousarray(tables, dtype=np.float32).reshape(-1)
        self.n_items, self.width = int(n_items), int(width)
        self.n_feat, self.n_rules = len(self.fields), len(self.rules)
        self.k = int(self.cols[:, 1].max()) + 1 if len(self.cols) else 0
        self._check()
        # the records the kernel walks: each group's rules in rank order with their itemsets' pair ranges
        ante, cons = self.sets[self.rules[self.order, 0]], self.sets[self.rules[self.order, 1]]
        self.scan = np.ascontiguousarray(np.stack([self.order, ante[..., 0], cons[..., 0],
                                                   ante[..., 1] | (cons[..., 1] << 8)], axis=-1), dtype=np.int32)
        self._device = {}

    def _check(self) -> None:
        if not 1 <= self.n_items <= MAX_ITEMS or not 1 <= self.n_rules <= MAX_RULES:
            raise ValueError(f"rule kernel handles 1 .. {MAX_ITEMS} items and 1 .. {MAX_RULES} rules, "
                             f"got {self.n_items} and {self.n_rules}")
        if not 1 <= self.n_feat <= MAX_FIELDS or self.width < 1:
            raise ValueError(f"rule kernel handles 1 .. {MAX_FIELDS} fields, got {self.n_feat}")
        if not 1 <= len(self.groups) <= MAX_GROUPS:
            raise ValueError(f"rule kernel handles 1 .. {MAX_GROUPS} scan groups, got {len(self.groups)}")
        if not 1 <= len(self.cols) <= MAX_COLUMNS or not 1 <= self.k <= MAX_RANK or (self.cols[:, 1] < 0).any():
            raise ValueError(f"rule kernel handles 1 .. {MAX_COLUMNS} columns of rank 1 .. {MAX_RANK}")
        geometry(self.n_feat, self.n_items)
        W = words(self.n_items)
        fd = self.fields
        if ((fd[:, 0] < FIELD_NONE) | (fd[:, 0] > FIELD_VALUES)).any() or (fd[:, 1:] < 0).any():
            raise ValueError("rule tables: a field record is malformed")
        used = fd[:, 0] != FIELD_NONE
        if (fd[used, 1] + fd[used, 2] > self.imap.size).any():
            raise ValueError("rule tables: a field's item map lies outside imap")
        num = fd[:, 0] == FIELD_VALUES
        if (fd[num, 3] + fd[num, 2] > self.nvals.size).any():
            raise ValueError("rule tables: a field's values lie outside nvals")
        for _, _, cnt, off in fd[num]:
            v = self.nvals[off:off + cnt]
            if not (v[1:] > v[:-1]).all():
                raise ValueError("rule tables: a numeric field's values are not strictly ascending")
        if (self.imap >= self.n_items).any() or (self.imap < -1).any():
            raise ValueError("rule tables: imap names an item outside the basket")
        s = self.sets
        if len(s) < 1 or (s < 0).any() or (s.sum(axis=1) > len(self.pairs)).any() or (s[:, 1] > 255).any():
            raise ValueError("rule tables: an itemset's pairs lie outside the pair table")
        if (self.pairs[:, 0] >= W).any():
            raise ValueError("rule tables: a pair names a word outside the basket")
        if ((self.rules < 0) | (self.rules >= len(s))).any():
            raise ValueError("rule tables: a rule names an itemset outside the set table")
        if self.order.shape != (len(self.groups), self.n_rules) \
                or ((self.order < 0) | (self.order >= self.n_rules)).any():
            raise ValueError("rule tables: a group's order is not a list of n_rules rule indices")
        g = self.groups
        if ((g[:, 0] < ALG_RECOMMENDATION) | (g[:, 0] > ALG_ASSOCIATION) | (g[:, 1] < 0) | (g[:, 1] > MAX_RANK)).any():
            raise ValueError("rule tables: a group's algorithm or rank count is out of range")
        c = self.cols
        if ((c[:, 0] < 0) | (c[:, 0] >= len(g))).any() \
                or ((c[:, 2] < 0) | (c[:, 2] + self.n_rules + 1 > self.tables.size)).any() \
                or ((c[:, 3] < 0) | (c[:, 3] >= self.width)).any():
            raise ValueError("rule tables: a column's group, table or destination is out of range")

    def on(self, device):
        """The tables as device tensors (cached per device)."""
        import torch

        key = str(device)
        d = self._device.get(key)
        if d is None:
            d = self._device[key] = {k: torch.from_numpy(getattr(self, k).view(np.int32) if k == "pairs"
                                                         else getattr(self, k)).to(device) for k in self._KERNEL}
        return d


def rules_launch(X, out, tables: RuleTables, prep=None, rows: Optional[int] = None, stream=None) -> None:
    """Device tensors: ``X`` fp32 ``[m, n_feat]`` (unit column stride, any row stride), ``out`` fp32
    ``[m, width]`` (unit column stride, any row stride): only the columns ``tables.cols`` names are
    written. ``prep``: the int32 ``FieldPrep`` table or None. ``rows`` overrides :func:`geometry`."""
    from . import _lib

    T = tables
    m = int(X.shape[0])
    if X.dim() != 2 or int(X.shape[1]) != T.n_feat or (T.n_feat > 1 and X.stride(1) != 1) \
            or (m > 1 and X.stride(0) < T.n_feat):
        raise ValueError(f"rules_launch needs a row-major [m, {T.n_feat}] X with unit column stride")
    if out.dim() != 2 or int(out.shape[0]) != m or int(out.shape[1]) != T.width \
            or (T.width > 1 and out.stride(1) != 1) or (m > 1 and out.stride(0) < T.width):
        raise ValueError(f"rules_launch needs a row-major [m, {T.width}] out with unit column stride")
    if prep is not None and (not prep.is_contiguous() or int(prep.numel()) < 8 * T.n_feat):
        raise ValueError("rules_launch needs a contiguous FieldPrep table of n_feat records")
    rows = geometry(T.n_feat, T.n_items) if rows is None else int(rows)
    if rows not in ROWS or lds_bytes(T.n_feat, T.n_items, rows) > LDS_BYTES:
        raise ValueError(f"rules_launch: {rows} rows per workgroup do not fit {LDS_BYTES} bytes of LDS")
    d = T.on(X.device)
    a = _lib.RuleArgs()
    a.X, a.prep, a.out = X.data_ptr(), (prep.data_ptr() if prep is not None else None), out.data_ptr()
    for k in T._KERNEL:
        setattr(a, k, d[k].data_ptr())
    a.n_rows, a.n_feat = m, T.n_feat
    a.ldx = int(X.stride(0)) if m > 1 else T.n_feat
    a.ldo = int(out.stride(0)) if m > 1 else T.width
    a.n_items, a.n_rules, a.n_group, a.n_col = T.n_items, T.n_rules, len(T.groups), len(T.cols)
    a.k, a.rows, a.n_tables, a.n_pair = T.k, rows, int(T.tables.size), len(T.pairs)
    a.n_map, a.n_vals = int(T.imap.size), int(T.nvals.size)
    _lib.check(_lib.load().pmml_rules_launch(_lib.stream_handle(stream), a), "pmml_rules_launch")


# --------------------------------------------------------------------------- numpy twin


def _inside(basket: np.ndarray, T: RuleTables, first: int, count: int) -> np.ndarray:
    """``rl_subset``: the itemset (``count`` pairs from ``first``) is a subset of each row's basket
    (``uint32 [n, W]``)."""
    r = np.ones(len(basket), dtype=bool)
    for w, mask in T.pairs[first:first + count]:
        r &= (basket[:, w] & mask) == mask
    return r


# The rule the tests' mutant replaces: under exclusiveRecommendation a rule is dropped when its WHOLE
# consequent is inside the basket.
_excluded = _inside


def rules_numpy(X: np.ndarray, out: np.ndarray, tables: RuleTables, prep: Optional[np.ndarray] = None,
                rows: Optional[int] = None, r: Optional[int] = None) -> np.ndarray:
    """The kernel on the host, tile by tile: writes the columns ``tables.cols`` names into ``out``
    (fp32 ``[m, width]``, in place) and returns it. ``r`` overrides the instantiation's slot count."""
    T = tables
    X = np.asarray(X, dtype=np.float32)
    m = int(X.shape[0])
    if X.ndim != 2 or X.shape[1] != T.n_feat or out.shape != (m, T.width) or out.dtype != np.float32:
        raise ValueError(f"rules_numpy needs X [m, {T.n_feat}] and a float32 out [m, {T.width}]")
    TB = geometry(T.n_feat, T.n_items) if rows is None else int(rows)
    R = template_r(T.k) if r is None else int(r)
    W = words(T.n_items)
    lanes_all = np.arange(TB)
    for r0 in range(0, m, TB):
        r1 = min(m, r0 + TB)
        n = r1 - r0
        lanes = lanes_all[:n]
        # stage_rows_T: the prepared planes and the rejected flags
        feat = np.empty((T.n_feat, n), dtype=np.float32)
        bad = np.zeros(n, dtype=bool)
        for f in range(T.n_feat):
            x = X[r0:r1, f]
            if prep is not None:
                bad |= prep_bad_numpy(x, prep, f)
                x = prep_numpy(x, prep, f)
            feat[f] = x
        ok = ~bad
        # the basket
        basket = np.zeros((n, W), dtype=np.uint32)
        for f in range(T.n_feat):
            kind, moff, cnt, voff = (int(v) for v in T.fields[f])
            if kind == FIELD_NONE:
                continue
            x = feat[f]
            item = np.full(n, -1, dtype=np.int64)
            with np.errstate(invalid="ignore"):
                if kind == FIELD_CODES:
                    inr = (x > np.float32(-1.0)) & (x < np.float32(cnt))
                    code = np.where(inr, x, 0).astype(np.int64)  # truncation toward zero
                    item = np.where(inr, T.imap[moff + code], -1)
                else:
                    vals = T.nvals[voff:voff + cnt]
                    lo = np.sum(vals[None, :] < x[:, None], axis=1)  # first value that is not below x
                    at = np.minimum(lo, max(cnt - 1, 0))
                    found = (lo < cnt) & (vals[at] == x) if cnt else np.zeros(n, dtype=bool)
                    item = np.where(found, T.imap[moff + at], -1)
            has = (item >= 0) & (item < T.n_items)
            w = np.where(has, item >> 5, 0)
            bit = np.where(has, np.uint32(1) << (item & 31).astype(np.uint32), 0).astype(np.uint32)
            basket[lanes, w] |= bit
        for g, (alg, need) in enumerate(T.groups):
            match = np.full((n, R), -1, dtype=np.int64)
            cnt_m = np.zeros(n, dtype=np.int64)
            for k, a0, c0, counts in T.scan[g]:
                if not (ok & (cnt_m < need)).any():
                    break  # every lane has the matches its columns read
                hit = ok & _inside(basket, T, a0, counts & 0xFF)
                if alg != ALG_RECOMMENDATION and hit.any():
                    if alg == ALG_EXCLUSIVE:
                        hit &= ~_excluded(basket, T, c0, (counts >> 8) & 0xFF)
                    else:
                        hit &= _inside(basket, T, c0, (counts >> 8) & 0xFF)
                for j in range(R):  # the register chain
                    match[:, j] = np.where(hit & (cnt_m == j), k, match[:, j])
                cnt_m += hit
            for cg, rank, off, dst in T.cols:
                if cg != g:
                    continue
                idx = match[:, rank] if rank < R else np.full(n, -1)
                out[r0:r1, dst] = T.tables[off + np.where(idx >= 0, idx, T.n_rules)]
    return out


__all__ = ["ALGORITHMS", "ALG_ASSOCIATION", "ALG_EXCLUSIVE", "ALG_RECOMMENDATION", "FIELD_CODES", "FIELD_NONE",
           "FIELD_VALUES", "LDS_BYTES", "MAX_COLUMNS", "MAX_FIELDS", "MAX_GROUPS", "MAX_ITEMS", "MAX_RANK", "MAX_RULES",
           "MAX_SET_ITEMS", "REG_WORDS", "ROWS", "RuleTables", "geometry", "lds_bytes", "rules_launch", "rules_numpy",
           "template_r", "words"]
