"""Lowering of a Scorecard's reason codes into the packed tables of ``ops/csrc/reasons.hip``.

:func:`lower_reasons` takes the ``ir.Scorecard``, the schema, the ``field_index`` of the kernel that
scores it (the general tree kernel's matrix: raw rows, or the tile of a derive pass with the
``__cps_<i>_<j>`` columns) and the ``reasonCode`` Output fields with their destination columns, and
returns a :class:`~flink_jpmml_amd.ops.reasons.ReasonTables`. It follows
``models/scorecard.py::_ReasonCodes._reason_codes``: the difference of a constant partial score is
formed here in float64 exactly as the oracle forms it; an attribute with a ``ComplexPartialScore``
carries its baseline and the column, and the kernel forms the difference from the fp32 value.

What the kernel cannot take raises :class:`NotLowerable` naming the Output field.
"""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from ..models.scorecard import complex_field
from ..ops import reasons as K
from ..pmml import ir
from .general_tree import _PredCompiler
from .plans import NotLowerable


def document_codes(sc: ir.Scorecard) -> Tuple[List[str], bool]:
    """The distinct reason codes in document order (an attribute's own code, else its
    characteristic's), and whether some code belongs to two characteristics."""
    codes: List[str] = []
    owner: Dict[str, int] = {}
    shared = False
    for i, ch in enumerate(sc.characteristics):
        for a in ch.attributes:
            code = a.reason_code or ch.reason_code
            if code is None:
                continue
            if code not in owner:
                owner[code] = i
                codes.append(code)
            elif owner[code] != i:
                shared = True
    return codes, shared


def check_baselines(sc: ir.Scorecard, first: ir.OutputField) -> None:
    """Every characteristic needs a baseline score, its own or the model's: without one the oracle
    raises ``UnsupportedFeatureException`` on every batch."""
    for i, ch in enumerate(sc.characteristics):
        if ch.baseline_score is None and sc.baseline_score is None:
            raise NotLowerable(f"output {first.name!r}: reason codes need a baselineScore "
                               f"(characteristic {ch.name or i!r} has none)")


def lower_reasons(sc: ir.Scorecard, schema, field_index: Dict[str, int], n_feat: int,
                  fields: List[Tuple[ir.OutputField, int]], width: int) -> K.ReasonTables:
    """``fields``: the ``reasonCode`` Output fields with their columns in the ``[rows, width]``
    output matrix."""
    if not fields:
        raise ValueError("lower_reasons needs at least one reasonCode field")
    first = fields[0][0]

    def no(of, why: str) -> NotLowerable:
        return NotLowerable(f"output {of.name!r}: {why}")

    for of, _ in fields:
        rank = max(1, int(of.rank))
        if rank > K.MAX_RANK:
            raise no(of, f"reason code rank {rank} > {K.MAX_RANK}")
    if len(fields) > K.MAX_COLUMNS:
        raise no(fields[K.MAX_COLUMNS][0], f"more than {K.MAX_COLUMNS} reasonCode fields")
    check_baselines(sc, first)
    codes, shared = document_codes(sc)
    if len(codes) > K.MAX_CODES:
        raise no(first, f"{len(codes)} distinct reason codes > {K.MAX_CODES}")
    if getattr(field_index, "folds", None):
        raise no(first, "reason codes need unfolded predicate columns")
    above = sc.reason_code_algorithm != "pointsBelow"
    index = {c: i for i, c in enumerate(codes)}
    pc = _PredCompiler(schema, field_index)
    chars, attrs, dval = [], [], []
    for i, ch in enumerate(sc.characteristics):
        base = ch.baseline_score if ch.baseline_score is not None else sc.baseline_score
        chars.append((len(attrs), len(ch.attributes)))
        for j, a in enumerate(ch.attributes):
            try:
                off = pc.compile(a.predicate)
            except NotLowerable as e:
                raise no(first, str(e)) from e
            code = a.reason_code or ch.reason_code
            vcol = -1
            if a.complex_score is not None:
                vcol = field_index.get(complex_field(i, j), -1)
                if vcol < 0:
                    raise no(first, f"the ComplexPartialScore column {complex_field(i, j)!r} is not a kernel input")
                d = float(base)
            else:
                partial = np.float64(a.partial_score)
                d = float((partial - np.float64(base)) if above else (np.float64(base) - partial))
            attrs.append((off, index[code] if code is not None else -1, vcol, 0))
            dval.append(d)
    n_code = max(1, len(codes))
    cols, tables = [], []
    for of, dst in fields:
        # every code of the document, in document order: the vocabulary is complete before the first batch
        enc = [float(schema.lookup(of.name, c)) for c in codes]
        cols.append((max(1, int(of.rank)) - 1, len(tables), dst, 0))
        tables.extend(enc + [float("nan")] * (n_code - len(enc)))
    try:
        K.geometry(n_feat, n_code, shared)
        return K.ReasonTables(chars, attrs, dval, pc.code, pc.pool or [0.0], cols, tables, n_code, n_feat, width,
                              above, shared)
    except ValueError as e:
        raise no(first, str(e)) from e


__all__ = ["check_baselines", "document_codes", "lower_reasons"]
