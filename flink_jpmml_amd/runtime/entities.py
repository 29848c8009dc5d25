"""Lowering of ranked-entity Output fields into the tables of ``ops/csrc/entities.hip``.

:func:`lower_entities` takes the ``ClusterPlan`` / ``KnnPlan`` that scores the model, its evaluator
and the ``entityId`` / ``clusterId`` / affinity Output fields with their destination columns, and
returns an :class:`~flink_jpmml_amd.ops.entities.EntityTables` over the plan's own fp32 tensors, so
the kernel repeats the plan's arithmetic. It follows ``models/base.py::_output_column``: a
ClusteringModel answers with its cluster ids and ranks up to ``min(K, 32)``, a NearestNeighborModel
with its training instance ids (never their targets) and ranks up to its ``k``; a rank past the list
is a NaN column.

What the kernel cannot take raises :class:`NotLowerable` naming the Output field.
"""

from __future__ import annotations

from typing import List, Tuple

import numpy as np

from ..ops import entities as K
from ..pmml import ir
from .plans import NotLowerable

ID_FEATURES = ("entityId", "clusterId")
AFFINITY_FEATURES = ("affinity", "clusterAffinity", "entityAffinity")
ENTITY_FEATURES = ID_FEATURES + AFFINITY_FEATURES


def entity_ids(ev) -> List[str]:
    """What ``entityId`` answers: training instance ids for a k-NN model, cluster ids otherwise."""
    return list(ev.instance_ids) if getattr(ev, "knn", None) is not None else list(ev.entity_ids)


def list_limit(ev) -> int:
    """The ranks the host keeps: the ``k`` neighbours, or ``min(K, 32)`` clusters."""
    n = len(ev.centers)
    return min(ev.k, n) if getattr(ev, "knn", None) is not None else min(n, K.MAX_RANK)


def is_entity_field(of: ir.OutputField, ev) -> bool:
    """Fields the entity kernel must write: every entity field of a k-NN model; of a
    ClusteringModel those of rank > 1 and the affinities that name a cluster (rank 1 stays a
    column of ``outputs_kernel``)."""
    if of.feature not in ENTITY_FEATURES:
        return False
    if getattr(ev, "knn", None) is not None or max(1, int(of.rank)) > 1:
        return True
    return of.feature in AFFINITY_FEATURES and of.value is not None and of.value in ev.entity_ids


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def lower_entities(plan, ev, schema, fields: List[Tuple[ir.OutputField, int]], width: int) -> K.EntityTables:
    """``plan``: the base ``ClusterPlan`` / ``KnnPlan``; ``fields``: the entity Output fields with
    their columns in the ``[rows, width]`` output matrix."""
    if not fields:
        raise ValueError("lower_entities needs at least one entity field")

    def no(of, why: str) -> NotLowerable:
        return NotLowerable(f"output {of.name!r}: {why}")

    knn_model = getattr(ev, "knn", None) is not None
    knn_plan = plan.kind == "knn"
    ent = _np(plan.inst if knn_plan else plan.centers)
    N, F = ent.shape
    first = fields[0][0]
    if F > K.MAX_FEATURES:
        raise no(first, f"entity ranks over {F} fields > {K.MAX_FEATURES}")
    if len(fields) > K.MAX_COLUMNS:
        raise no(fields[K.MAX_COLUMNS][0], f"more than {K.MAX_COLUMNS} entity columns")
    ids = entity_ids(ev)
    if len(ids) != N:
        raise no(first, f"{len(ids)} entity ids for {N} entities")
    limit = list_limit(ev)
    cols, tables = [], []
    named = np.full(N, -1, dtype=np.int32)
    top = 1
    for j, (of, dst) in enumerate(fields):
        rank = max(1, int(of.rank))
        if rank > K.MAX_RANK:
            raise no(of, f"entity rank {rank} > {K.MAX_RANK}")
        if of.feature in AFFINITY_FEATURES and of.value is not None and of.value in ids:
            if knn_model:
                raise no(of, f"{of.feature} of the named training instance {of.value!r} is not kept "
                             f"(only the k nearest are)")
            e = ids.index(of.value)
            if named[e] < 0:
                named[e] = j
            cols.append((K.ENT_NAMED, e, 0, dst))
            continue
        top = max(top, min(rank, limit))
        if of.feature in AFFINITY_FEATURES:
            cols.append((K.ENT_AFFINITY, rank - 1, 0, dst))
            continue
        if of.feature == "clusterId":
            enc = [i + 1.0 for i in range(N)]
        else:
            enc = [float(schema.lookup(of.name, x)) for x in ids]
        if any(float(np.float32(v)) != v for v in enc):
            raise no(of, "an entity id whose encoding fp32 cannot hold exactly")
        cols.append((K.ENT_ID, rank - 1, len(tables), dst))
        tables.extend(enc)
    k = int(plan.k) if knn_plan else top
    mfma = plan.variant == "mfma"
    try:
        return K.EntityTables(ent, _np(plan.weights), _np(plan.scales), _np(plan.qweights), _np(plan.cfun),
                              int(plan.metric_code), bool(plan.similarity), float(plan.p), cols, named, tables, k,
                              knn_plan, width, wc=_np(plan.wc) if mfma else None, cc=_np(plan.cc) if mfma else None)
    except ValueError as e:
        raise no(first, str(e)) from e


__all__ = ["AFFINITY_FEATURES", "ENTITY_FEATURES", "ID_FEATURES", "entity_ids", "is_entity_field", "list_limit",
           "lower_entities"]
