"""Lowering of an AssociationModel's ``ruleValue`` / ``entityId`` Output fields into the packed tables
of ``ops/csrc/rules.hip``.

:func:`lower_rules` takes the ``AssociationEvaluator``, the schema, the active fields (the columns of
the raw matrix) and the rule Output fields with their destination columns, and returns a
:class:`~flink_jpmml_amd.ops.rules.RuleTables`. It follows ``models/association.py``:

* **items**: one basket bit per distinct item value, in document order. A string field maps its
  vocabulary codes to items (it must declare its values: an open vocabulary grows with the records,
  and a code registered after lowering could name an item); a numeric field holds the sorted fp32 values ``v`` whose text
  ``_fmt(float(v))`` is an item value as written: the oracle applied to ``float32(x)``. ``"0.1"`` or
  ``"3.0"`` can never be in a basket built from such a field and are left out;
* **scan groups**: per distinct ``(algorithm, rankBasis, rankOrder)`` the rule indices sorted with
  the oracle's key, so the kernel's ``r``-th match is the rank-``r`` rule;
* **columns**: per Output field a ``[n_rules + 1]`` fp32 table, NaN last: ``np.float32`` of a measure
  (NaN where the rule lacks it), ``schema.lookup`` of a string feature, registered in rule order with
  the field typed as string as the oracle does.

What the kernel cannot take raises :class:`NotLowerable` naming the Output field.
"""

from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np

from ..models.association import _MEASURES, _fmt
from ..ops import rules as K
from ..pmml import ir
from .plans import NotLowerable

RULE_FEATURES = ("ruleValue", "entityId")
STRING_FEATURES = ("antecedent", "consequent", "rule", "ruleId")


def rule_feature(of: ir.OutputField) -> str:
    """What the field reports of its rule: ``entityId`` is the rule's id."""
    return "ruleId" if of.feature == "entityId" else of.rule_feature


def rule_rank(of: ir.OutputField) -> int:
    return of.rank if of.rank and of.rank > 0 else 1


def scan_group(of: ir.OutputField) -> Tuple[str, str, bool]:
    """``(algorithm, rank basis, ascending)`` as ``AssociationEvaluator._ranked`` reads them."""
    basis = of.rank_basis if of.rank_basis in _MEASURES else "confidence"
    return of.algorithm, basis, of.rank_order == "ascending"


def group_order(rules: List[ir.AssociationRule], basis: str, ascending: bool) -> List[int]:
    """The rule indices under the oracle's sort key: ``sign * measure``, a missing measure as
    ``-inf``, document order on ties."""
    sign = 1.0 if ascending else -1.0

    def key(k):
        v = getattr(rules[k], basis)
        return (sign * (v if v is not None else -math.inf), k)

    return sorted(range(len(rules)), key=key)


def numeric_items(texts: List[str]) -> List[Tuple[np.float32, str]]:
    """The fp32 values that name an item of a numeric field, ascending, with the item's text."""
    out = []
    for t in texts:
        try:
            with np.errstate(over="ignore"):
                v = np.float32(float(t))
        except (TypeError, ValueError):
            continue
        if _fmt(float(v)) == t:
            out.append((v, t))
    return sorted(set(out), key=lambda p: float(p[0]))


def rule_texts(ev, feature: str) -> List[str]:
    """``AssociationEvaluator._rule_value`` of a string feature for every rule, in rule order. A rule
    without an id answers with the 1-based position of the first rule equal to it, as
    ``list.index`` does there."""
    if feature != "ruleId":
        return [ev._rule_value(r, feature) for r in ev.rules]
    first: Dict[tuple, int] = {}
    out = []
    for k, r in enumerate(ev.rules):
        key = (r.antecedent, r.consequent, r.support, r.confidence, r.lift, r.leverage, r.affinity, r.rule_id)
        first.setdefault(key, k)
        out.append(r.rule_id if r.rule_id is not None else str(first[key] + 1))
    return out


def lower_rules(ev, compiled, fields: List[Tuple[ir.OutputField, int]], width: int) -> K.RuleTables:
    """``fields``: the ``ruleValue`` / ``entityId`` Output fields with their columns in the
    ``[rows, width]`` output matrix."""
    if not fields:
        raise ValueError("lower_rules needs at least one rule field")
    schema = compiled.schema
    active = list(compiled.active_fields)
    first = fields[0][0]

    def no(of, why: str) -> NotLowerable:
        return NotLowerable(f"output {of.name!r}: {why}")

    for of, _ in fields:
        if of.algorithm not in K.ALGORITHMS:
            raise no(of, f"association algorithm {of.algorithm!r}")
        if rule_feature(of) not in STRING_FEATURES + _MEASURES:
            raise no(of, f"association ruleFeature {rule_feature(of)!r}")
        if rule_rank(of) > K.MAX_RANK:
            raise no(of, f"rule rank {rule_rank(of)} > {K.MAX_RANK}")
    if len(fields) > K.MAX_COLUMNS:
        raise no(fields[K.MAX_COLUMNS][0], f"more than {K.MAX_COLUMNS} rule columns")
    rules = ev.rules
    if not rules:
        raise no(first, "the document has no rules")
    if len(rules) > K.MAX_RULES:
        raise no(first, f"{len(rules)} rules > {K.MAX_RULES}")
    if not 1 <= len(active) <= K.MAX_FIELDS:
        raise no(first, f"{len(active)} active fields, the rule kernel takes 1 .. {K.MAX_FIELDS}")

    # items: one bit per distinct value, document order
    item: Dict[str, int] = {}
    for v in ev.model.items.values():
        item.setdefault(v, len(item))
    if len(item) > K.MAX_ITEMS:
        raise no(first, f"{len(item)} items > {K.MAX_ITEMS}")
    n_items = max(1, len(item))

    # itemsets, word-sparse; only those a rule names
    set_index: Dict[str, int] = {}
    sets, pairs = [], []
    for r in rules:
        for sid in (r.antecedent, r.consequent):
            if sid in set_index:
                continue
            members = ev.sets[sid]
            if len(members) > K.MAX_SET_ITEMS:
                raise no(first, f"itemset {sid!r} has {len(members)} items > {K.MAX_SET_ITEMS}")
            masks: Dict[int, int] = {}
            for v in members:
                masks[item[v] >> 5] = masks.get(item[v] >> 5, 0) | (1 << (item[v] & 31))
            set_index[sid] = len(sets)
            sets.append((len(pairs), len(masks)))
            pairs.extend(sorted(masks.items()))
    rule_table = [(set_index[r.antecedent], set_index[r.consequent]) for r in rules]

    # per active field: the fp32 value of a prepared row -> the item it names
    frec, imap, nvals = [], [], []
    for f in active:
        if schema.is_string(f):
            df = schema.data_fields.get(f)
            if df is None or not df.values:
                # an open vocabulary grows with the records: a code registered after lowering could name an item
                raise no(first, f"field {f!r}: a string field without declared values is host-only")
            vocab = list(schema.values.get(f, []))
            frec.append((K.FIELD_CODES, len(imap), len(vocab), 0))
            imap.extend(item.get(v, -1) for v in vocab)
            continue
        dtype = schema.types.get(f)
        mf = compiled.mining_fields.get(f)
        if dtype == "boolean":
            raise no(first, f"field {f!r}: the items of a boolean field are host-only")
        if dtype == "integer" and mf is not None and mf.invalid_value_treatment == "asIs":
            raise no(first, f"field {f!r}: an integer field that keeps non-integral values (asIs) is host-only")
        found = numeric_items(list(item))
        frec.append((K.FIELD_VALUES if found else K.FIELD_NONE, len(imap), len(found), len(nvals)))
        imap.extend(item[t] for _, t in found)
        nvals.extend(v for v, _ in found)

    # scan groups and columns
    group_index: Dict[tuple, int] = {}
    groups, order, cols, tables = [], [], [], []
    for of, dst in fields:
        key = scan_group(of)
        g = group_index.get(key)
        if g is None:
            if len(groups) == K.MAX_GROUPS:
                raise no(of, f"more than {K.MAX_GROUPS} distinct (algorithm, rankBasis, rankOrder)")
            g = group_index[key] = len(groups)
            groups.append([K.ALGORITHMS[key[0]], 0])
            order.append(group_order(rules, key[1], key[2]))
        rank = rule_rank(of)
        groups[g][1] = max(groups[g][1], rank)
        feature = rule_feature(of)
        if feature in _MEASURES:
            enc = [np.float32(np.nan) if getattr(r, feature) is None else np.float32(getattr(r, feature))
                   for r in rules]
        else:
            schema.types.setdefault(of.name, "string")
            vals = [float(schema.lookup(of.name, t)) for t in rule_texts(ev, feature)]
            if any(float(np.float32(v)) != v for v in vals):
                raise no(of, "a rule text whose encoding fp32 cannot hold exactly")
            enc = [np.float32(v) for v in vals]
        cols.append((g, rank - 1, len(tables), dst))
        tables.extend(enc + [np.float32(np.nan)])
    try:
        return K.RuleTables(frec, imap, nvals, sets, pairs, rule_table, order, groups, cols, tables, n_items, width)
    except ValueError as e:
        raise no(first, str(e)) from e


__all__ = ["RULE_FEATURES", "STRING_FEATURES", "group_order", "lower_rules", "numeric_items", "rule_feature",
           "rule_rank", "rule_texts", "scan_group"]
