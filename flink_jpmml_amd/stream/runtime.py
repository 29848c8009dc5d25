"""A deterministic dataflow runtime with Flink's operator semantics — in one process, or one
process per GPU under ``torchrun`` (SPMD data parallelism over RCCL / gloo).

The reference runs on Apache Flink (TaskManagers, network stack, checkpoints). This runtime keeps
exactly the semantics the reference's operators depend on:

* a job graph of sources, one-input operators (map / flat_map / filter / process), two-input
  operators (``connect`` + ``broadcast``) and sinks;
* per-operator **parallelism**: every subtask holds its own operator instance — one model
  replica per subtask, like Flink (`S/api/functions/EvaluationFunction.scala:43`). In one process
  the subtasks are copies routed ``forward`` / ``rebalance`` / ``broadcast``; **under torchrun
  every rank is one subtask of every operator** (parallelism = world size, one GPU each): event
  sources are sharded by rank, broadcast (control) streams are replicated to every rank, model
  loads parse once on rank 0 and replicate the compiled tensors (SURVEY §2.6 F1–F5);
* **live, available-first input** (:mod:`~flink_jpmml_amd.stream.inputs`): sources that can block
  (sockets, paced generators, push sources, leader-read streams) run on reader threads and the job
  thread processes whichever input has data — an idle control stream never holds events back.
  Bounded, non-blocking sources and timestamped test harnesses keep a **deterministic merge** (by
  timestamp when every source provides one, else round-robin — the analogue of
  `T/sources/TemporizedSourceFunction.scala:35-56`);
* **processing-time timers** on the job :class:`~flink_jpmml_amd.stream.clock.Clock` (latency
  bound micro-batches flush while a slow source sleeps);
* **checkpoints** with **source offsets**, either **time-based** (``interval_ms``, the reference's
  ``enableCheckpointing(ms)``, `E/DynamicEvaluateKmeans.scala:48`; across ranks rank 0 decides and
  the :class:`~flink_jpmml_amd.stream.coordinator.CheckpointCoordinator` injects the barrier into
  every rank's input) or **count-based** (barriers on the primary source's global offset, aligned
  across ranks without communication). Offsets are what each rank *processed* before the barrier
  (an exact cut, per rank). ``CheckpointedFunction``s snapshot into operator state (union /
  split list state); rank 0 writes one JSON manifest (operator state of every subtask, source
  offsets, sha256 of every served model); transactional sinks pre-commit at the barrier and
  commit after the manifest is durable. ``execute(restore=…)`` re-broadcasts the manifest,
  re-initialises operators (`S/api/functions/EvaluationCoFunction.scala:76-96`) and resumes every
  source at its offset: outputs of a restarted job equal an uninterrupted run's (exactly-once);
* failures inside operators abort the job with :class:`JobExecutionException` (Flink's
  ``JobExecutionException`` in the reference's tests, `T/RichDataStreamSpec.scala:82-89`).
"""

from __future__ import annotations

import bisect
import copy
import logging
import time
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Iterator, List, Optional, Tuple

from ..api.batch import RecordBatch
from ..utils.metrics import METRICS
from ..utils.profiling import prange
from .clock import Clock, SystemClock, set_current_clock
from .functions import (
    CheckpointedFunction,
    Collector,
    FunctionInitializationContext,
    FunctionSnapshotContext,
    ProcessContext,
    RichFunction,
    RuntimeContext,
    SinkFunction,
)
from .inputs import Chunk
from .sources import SourceReader
from .state import CheckpointStorage, OperatorStateStore

logger = logging.getLogger(__name__)


class JobExecutionException(RuntimeError):
    """The job failed; ``__cause__`` is the operator's exception."""


class SimulatedFailure(RuntimeError):
    """Raised by the fault-injection hook (:meth:`StreamExecutionEnvironment.inject_failure`)."""


@dataclass
class Node:
    kind: str  # source | one | two | sink
    name: str
    parallelism: int
    factory: Any = None  # operator prototype (deep-copied per subtask)
    inputs: List[Tuple["Node", str]] = field(default_factory=list)  # (upstream, partitioning)
    source: Any = None
    timestamp_fn: Optional[Callable[[Any], Any]] = None
    uid: str = ""
    op_kind: str = ""  # map | flat_map | filter | process | co_process | sink
    dist_mode: str = "shard"  # sources under torchrun: shard | replicate | either | parallel

    def __hash__(self) -> int:
        return id(self)


@dataclass
class JobExecutionResult:
    job_name: str
    net_runtime_ms: float
    records_in: int
    checkpoints: List[str]
    accumulators: Dict[str, Any] = field(default_factory=dict)
    elements_in: int = 0
    input_mode: Optional[str] = None


def _encode_state(x: Any) -> Any:
    """JSON encoding of state items: dicts keyed by ModelId become lists of entries."""
    from ..domain.model_id import ModelId, ModelInfo

    if isinstance(x, dict) and x and all(isinstance(k, ModelId) for k in x):
        return {"__metadata__": [{"name": k.name, "version": k.version, "path": v.path if isinstance(v, ModelInfo)
                                  else str(v)} for k, v in x.items()]}
    return x


def _decode_state(x: Any) -> Any:
    from ..domain.model_id import ModelId, ModelInfo

    if isinstance(x, dict) and "__metadata__" in x:
        return {ModelId(e["name"], int(e["version"])): ModelInfo(e["path"]) for e in x["__metadata__"]}
    return x


class _Subtask:
    def __init__(self, node: Node, index: int, op: Any):
        self.node = node
        self.index = index
        self.op = op
        self.out: Optional[Collector] = None
        self.rr = 0


class Executor:
    def __init__(self, env: "StreamExecutionEnvironment", sinks: List[Node], restore: Optional[str]):
        self.env = env
        self.sinks = sinks
        self.restore = restore
        self.dist = env.dist_ctx if env.dist_ctx is not None and env.dist_ctx.is_distributed else None
        self.rank = self.dist.rank if self.dist else 0
        self.world = self.dist.world_size if self.dist else 1
        self.clock: Clock = env.clock or SystemClock()
        self.nodes: List[Node] = self._topo(sinks)
        self.down: Dict[int, List[Tuple[Node, str, int]]] = {id(n): [] for n in self.nodes}
        for n in self.nodes:
            for port, (up, part) in enumerate(n.inputs):
                self.down[id(up)].append((n, part, port))
        self.subtasks: Dict[int, List[_Subtask]] = {}
        self.records_in = 0  # rows (a RecordBatch counts its rows)
        self.elements_in = 0  # stream elements
        self.checkpoint_paths: List[str] = []
        self.readers: Dict[int, SourceReader] = {}
        self.processed: Dict[int, int] = {}  # per source: next global offset after what was processed
        self.primary: Optional[Node] = None
        self.next_cid = 1
        self.watchdog = None
        self.coordinator = None
        self._next_due: Optional[float] = None

    @staticmethod
    def _topo(sinks: List[Node]) -> List[Node]:
        order: List[Node] = []
        seen = set()

        def visit(n: Node) -> None:
            if id(n) in seen:
                return
            seen.add(id(n))
            for up, _ in n.inputs:
                visit(up)
            order.append(n)

        for s in sinks:
            visit(s)
        return order

    def _parallelism(self, n: Node) -> int:
        return self.world if self.dist else n.parallelism

    # ------------------------------------------------------------------ setup
    def _restored_doc(self) -> dict:
        if not self.restore:
            return {}
        doc = None
        if self.rank == 0:
            doc = CheckpointStorage.read(self.restore)
        if self.dist:  # rank 0 reads the manifest and re-broadcasts it (F4)
            from ..parallel.dist import broadcast_object

            doc = broadcast_object(doc, self.dist, group=self.dist.group("ctrl"))
        return doc or {}

    def _instantiate(self, doc: dict) -> None:
        restored_state: Dict[str, Dict[str, dict]] = doc.get("operators", {})
        for n in self.nodes:
            p = self._parallelism(n)
            if self.dist:
                indices = [self.rank]  # SPMD: this process is subtask `rank` of every operator
            else:
                indices = list(range(n.parallelism))
            subs = []
            for i in indices:
                op = None
                if n.kind in ("one", "two", "sink"):
                    op = n.factory if len(indices) == 1 and not self.env.copy_operators else _clone(n.factory)
                subs.append(_Subtask(n, i, op))
            self.subtasks[id(n)] = subs
            for st in subs:
                op = st.op
                rctx = RuntimeContext(n.name, st.index, p, clock=self.clock, dist=self.dist, config=self.env.config)
                if isinstance(op, RichFunction):
                    op.set_runtime_context(rctx)
                if isinstance(op, CheckpointedFunction):
                    restored = None
                    snap = restored_state.get(n.uid)
                    if snap is not None:
                        restored = {}
                        for name, entries in snap.items():
                            mode = entries.get("mode", "union")
                            parts = entries.get("subtasks", [])
                            flat = [_decode_state(x) for part in parts for x in part]
                            # union: every subtask gets all entries; split: round-robin redistribution
                            restored[name] = flat if mode == "union" else flat[st.index::p]
                    store = OperatorStateStore(restored)
                    op._state_store = store
                    op.initialize_state(FunctionInitializationContext(store, restored is not None))
                if isinstance(op, SinkFunction):
                    op.open(rctx)
                    if self.restore and hasattr(op, "recover"):
                        op.recover(doc.get("checkpoint_id"))
        for n in self.nodes:
            for st in self.subtasks[id(n)]:
                st.out = Collector(self._emitter(n, st), self._emitter_many(n, st))
                if isinstance(st.op, RichFunction):
                    st.op.open({})

    # ------------------------------------------------------------------ routing
    def _emitter(self, node: Node, st: _Subtask) -> Callable[[Any], None]:
        downs = self.down[id(node)]

        def emit(value: Any) -> None:
            for dn, part, port in downs:
                subs = self.subtasks[id(dn)]
                if part == "broadcast" or len(subs) == 1:
                    targets = subs
                elif part == "forward" and len(subs) == len(self.subtasks[id(node)]):
                    targets = [subs[st.index % len(subs)]]
                else:  # rebalance
                    targets = [subs[st.rr % len(subs)]]
                    st.rr += 1
                for t in targets:
                    self._deliver(dn, t, port, value)

        return emit

    def _emitter_many(self, node: Node, st: _Subtask) -> Callable[[list], None]:
        downs = self.down[id(node)]

        if len(downs) > 1:  # fan-out: branches may merge again downstream (from_either's split
            emit = self._emitter(node, st)  # into events + control): keep element order across them

            def emit_each(values: list) -> None:
                for v in values:
                    emit(v)

            return emit_each

        def emit_many(values: list) -> None:
            if not values:
                return
            for dn, part, port in downs:
                subs = self.subtasks[id(dn)]
                if part == "broadcast" or len(subs) == 1:
                    for t in subs:
                        self._deliver_many(dn, t, port, values)
                elif part == "forward" and len(subs) == len(self.subtasks[id(node)]):
                    self._deliver_many(dn, subs[st.index % len(subs)], port, values)
                else:  # rebalance: element-wise round robin
                    for v in values:
                        self._deliver(dn, subs[st.rr % len(subs)], port, v)
                        st.rr += 1

        return emit_many

    def _deliver_many(self, node: Node, st: _Subtask, port: int, values: list) -> None:
        """Chunked delivery: one call per chunk for map / filter / plain functions and for
        operators implementing the ``*_many`` hooks (order and results are those of element-wise
        delivery; operators keeping a collector for later, e.g. timers, always get ``st.out``)."""
        op = st.op
        k = node.op_kind
        if k == "map":
            f = op.map if hasattr(op, "map") else op
            st.out.collect_many([f(v) for v in values])
        elif k == "filter":
            f = op.filter if hasattr(op, "filter") else op
            st.out.collect_many([v for v in values if f(v)])
        elif k in ("flat_map", "process"):
            many = getattr(op, "flat_map_many", None)
            if many is not None:
                many(values, st.out)
            elif hasattr(op, "flat_map"):
                for v in values:
                    op.flat_map(v, st.out)
            else:
                res: list = []
                for v in values:
                    res.extend(op(v))
                st.out.collect_many(res)
        elif k == "co_process":
            many = getattr(op, "process_elements1", None) if port == 0 else None
            if many is not None:
                many(values, ProcessContext(None), st.out)
            else:
                for v in values:
                    self._deliver(node, st, port, v)
        elif k == "sink":
            many = getattr(op, "invoke_many", None)
            if many is not None:
                many(values)
            else:
                inv = op.invoke if hasattr(op, "invoke") else op
                for v in values:
                    inv(v)
        else:  # pragma: no cover
            raise RuntimeError(f"unknown operator kind {k}")

    def _deliver(self, node: Node, st: _Subtask, port: int, value: Any) -> None:
        op = st.op
        k = node.op_kind
        if k == "map":
            st.out.collect(op.map(value) if hasattr(op, "map") else op(value))
        elif k == "filter":
            keep = op.filter(value) if hasattr(op, "filter") else op(value)
            if keep:
                st.out.collect(value)
        elif k in ("flat_map", "process"):
            if hasattr(op, "flat_map"):
                op.flat_map(value, st.out)
            else:
                for v in op(value):
                    st.out.collect(v)
        elif k == "co_process":
            ctx = ProcessContext(None)
            if port == 0:
                op.process_element1(value, ctx, st.out)
            else:
                op.process_element2(value, ctx, st.out)
        elif k == "sink":
            op.invoke(value) if hasattr(op, "invoke") else op(value)
        else:  # pragma: no cover
            raise RuntimeError(f"unknown operator kind {k}")

    # ------------------------------------------------------------------ sources
    def _open_readers(self, doc: dict) -> List[Node]:
        sources = [n for n in self.nodes if n.kind == "source"]
        saved = doc.get("sources", {})
        for n in sources:
            entry = saved.get(n.uid, {})
            off = int(entry.get("offset", 0))
            ranks = entry.get("ranks")
            leader = None
            # earlier rescales' owner cuts still in force when that checkpoint was taken
            cuts = [[int(c) for c in lay] for lay in entry.get("skip_layers", [])] or None
            if ranks is not None and len(ranks) == self.world:
                off = int(ranks[self.rank])  # per-rank cut of a time-based checkpoint
                leader = int(min(ranks))
            elif ranks is not None:
                # rescaled restore of a time-based checkpoint: every rank stopped at its own cut
                if n.dist_mode in ("parallel", "either"):
                    raise RuntimeError(f"source {n.uid}: checkpoint was taken at world size {len(ranks)}, "
                                       f"restoring at {self.world} needs the same rank-local splits")
                off = int(min(ranks))
                if n.dist_mode == "shard":
                    # old rank j owned the global offsets g with g % old_world == j and processed
                    # those below its cut: resume at the smallest cut, skip what its owner did
                    cuts = (cuts or []) + [[int(r) for r in ranks]]
                # replicate / all: every rank saw every element; replaying from the smallest cut
                # re-applies control messages the union-restored state already holds (Add of a
                # known id is ignored, Del of an absent one is a no-op: MetadataManager)
            self.readers[id(n)] = SourceReader(n, self.rank, self.world, self.clock, off, leader_offset=leader,
                                               owner_cuts=cuts)
            self.processed[id(n)] = off
        primaries = [n for n in sources if n.dist_mode != "replicate"] or sources
        self.primary = primaries[0] if primaries else None
        if self.env.checkpoint_every and self.primary is not None:
            done = self.readers[id(self.primary)].offset // self.env.checkpoint_every
            self.next_cid = done + 1
        elif doc.get("checkpoint_id") is not None:
            self.next_cid = int(doc["checkpoint_id"]) + 1
        return sources

    def _input_mode(self, sources: List[Node]) -> str:
        from .clock import ManualClock
        from .inputs import is_live_source

        mode = getattr(self.env, "input_mode", "auto")
        if mode != "auto":
            return mode
        if isinstance(self.clock, ManualClock):
            return "deterministic"  # virtual time lives on the job thread
        if self.env.checkpoint_interval_ms and self.dist:
            return "live"  # barriers arrive from the coordinator thread
        return "live" if any(is_live_source(n.source) for n in sources) else "deterministic"

    def _check_checkpoint_config(self, sources: List[Node], mode: str) -> None:
        every = self.env.checkpoint_every
        if not every or not self.dist:
            return
        prim = self.primary
        if prim is not None and prim.dist_mode == "parallel":
            raise ValueError("count-based checkpoints need a globally numbered primary source (shard / either "
                             "mode); rank-local sources have per-rank lengths: use enable_checkpointing(interval_ms=…)")
        if mode == "live":
            raise ValueError("count-based checkpoints across ranks need deterministic input; live sources "
                             "checkpoint on time: use enable_checkpointing(interval_ms=…)")

    # ------------------------------------------------------------------ checkpoints
    def _maybe_checkpoint(self, upto: int) -> None:
        """Take every count-based checkpoint whose barrier offset is <= ``upto`` (primary-source
        global offset)."""
        every = self.env.checkpoint_every
        if not every:
            return
        while self.next_cid * every <= upto:
            self._checkpoint(self.next_cid, barrier=self.next_cid * every)
            self.next_cid += 1

    def _time_checkpoint_due(self) -> None:
        """Single-process time-based checkpoints: taken between elements on the job thread."""
        iv = self.env.checkpoint_interval_ms
        if not iv or self.coordinator is not None:
            return
        now = self.clock.now()
        if self._next_due is None:
            self._next_due = now + iv / 1e3
        elif now >= self._next_due:
            self._checkpoint(self.next_cid)
            self.next_cid += 1
            self._next_due = self.clock.now() + iv / 1e3

    def _checkpoint(self, cid: int, barrier: Optional[int] = None) -> None:
        with prange("checkpoint"):
            t0 = time.perf_counter()
            for n in self.nodes:  # flush buffered micro-batches / in-flight scores in topological order
                for st in self.subtasks[id(n)]:
                    if hasattr(st.op, "on_barrier"):
                        st.op.on_barrier(st.out)
            operators: Dict[str, Dict[str, dict]] = {}
            models: Dict[str, dict] = {}
            for n in self.nodes:
                subs = self.subtasks[id(n)]
                for st in subs:
                    if hasattr(st.op, "checkpoint_models"):
                        models.update(st.op.checkpoint_models())
                if not subs or not isinstance(subs[0].op, CheckpointedFunction):
                    continue
                per_state: Dict[str, dict] = {}
                for st in subs:
                    st.op.snapshot_state(FunctionSnapshotContext(cid, int(time.time() * 1000)))
                    snap = st.op._state_store.snapshot(_encode_state)
                    for name, s in snap.items():
                        e = per_state.setdefault(name, {"mode": s["mode"], "subtasks": []})
                        e["subtasks"].append(s["items"])
                operators[n.uid] = per_state
            # source positions = what this rank has *processed* (never what a reader buffered)
            local_src: Dict[str, int] = {}
            for n in self.nodes:
                if n.kind == "source":
                    local_src[n.uid] = barrier if (barrier is not None and n is self.primary) else \
                        self.processed[id(n)]
            sinks = [st.op for n in self.nodes if n.kind == "sink" for st in self.subtasks[id(n)]]
            for sk in sinks:
                if hasattr(sk, "pre_commit"):
                    sk.pre_commit(cid)
            if self.dist:
                from ..parallel.dist import broadcast_object, gather_object
                from ..utils.faults import guarded_collective

                g = self.dist.group("ctrl")
                parts = guarded_collective(gather_object, (operators, models, local_src), self.dist, group=g,
                                           what=f"checkpoint {cid} state gather")
                path = None
                if self.rank == 0:
                    merged_ops: Dict[str, Dict[str, dict]] = {}
                    for ops, mods, _ in parts:  # rank order = subtask order
                        models.update(mods)
                        for uid, states in ops.items():
                            for name, s in states.items():
                                e = merged_ops.setdefault(uid, {}).setdefault(name, {"mode": s["mode"],
                                                                                     "subtasks": []})
                                e["subtasks"].extend(s["subtasks"])
                    sources = {}
                    for uid, off in local_src.items():
                        ranks = [p[2][uid] for p in parts]
                        sources[uid] = self._skip_layers(uid, {"offset": off, "ranks": ranks}, ranks)
                    path = self._write_manifest(cid, merged_ops, sources, models)
                path = guarded_collective(broadcast_object, path, self.dist, group=g,
                                          what=f"checkpoint {cid} commit")
            else:
                sources = {uid: self._skip_layers(uid, {"offset": off}, [off]) for uid, off in local_src.items()}
                path = self._write_manifest(cid, operators, sources, models)
            for sk in sinks:
                if hasattr(sk, "commit"):
                    sk.commit(cid)
            self.checkpoint_paths.append(path)
            METRICS.inc("checkpoint.completed")
            METRICS.observe("checkpoint.duration_ms", (time.perf_counter() - t0) * 1e3)

    def _skip_layers(self, uid: str, entry: dict, ranks: List[int]) -> dict:
        """Carry a rescaled restore's owner cuts into the next checkpoint while some reader is still
        inside their skip window: a cut list stays until ``min(ranks)`` has passed its
        largest cut, since a restore from this checkpoint resumes at ``min(ranks)`` and must not
        re-score what the old owners had already processed."""
        rd = next((r for r in self.readers.values() if r.node.uid == uid), None)
        lo = min(ranks) if ranks else 0
        live = [lay for lay in (getattr(rd, "skip_layers", None) or []) if max(lay) > lo]
        if live:
            entry["skip_layers"] = live
        return entry

    def _write_manifest(self, cid: int, operators, sources, models) -> str:
        payload = {"operators": operators, "sources": sources, "models": models, "records_in": self.records_in,
                   "world_size": self.world,
                   "trigger": "count" if self.env.checkpoint_every else "time"}
        return self.env.checkpoint_storage.write(cid, payload)

    # ------------------------------------------------------------------ run
    def _finish_input(self, inputs) -> None:
        """End of input: align the last checkpoints across ranks, flush every operator, commit
        sinks."""
        if self.env.checkpoint_every and self.primary is not None:
            # the final global offset is known locally (strided sources report their global
            # length, filtered ones read everything): no collective that could interleave with a
            # peer's last in-stream checkpoint
            self._maybe_checkpoint(self.readers[id(self.primary)].offset)
        if self.coordinator is not None:
            # a finished rank keeps taking the checkpoints its peers trigger until all are done
            self.coordinator.finish_input()
            for m in inputs.markers():
                if self.watchdog is not None:
                    self.watchdog.kick()
                if m.kind == "barrier":
                    self._checkpoint(m.cid)
                    self.next_cid = m.cid + 1
                elif m.kind == "error":
                    raise m.exc
                elif m.kind == "stop":
                    break
                self.clock.fire_due()
        for n in self.nodes:  # flush buffered micro-batches, in topological order
            for st in self.subtasks[id(n)]:
                if hasattr(st.op, "end_of_input"):
                    st.op.end_of_input(st.out)
        for n in self.nodes:
            if n.kind == "sink":
                for st in self.subtasks[id(n)]:
                    if hasattr(st.op, "pre_commit"):
                        st.op.pre_commit(-1)
                    if hasattr(st.op, "commit"):
                        st.op.commit(-1)

    def _gc_tune(self):
        """Per-record streams allocate a few objects per record; CPython's cyclic collector would
        rescan every live object (inputs, buffered outputs) again and again. During the job the
        objects that existed before it are frozen out of collection and young collections run
        every 50k allocations (``env.gc_tuning = False`` keeps the interpreter defaults)."""
        if not getattr(self.env, "gc_tuning", True):
            return None
        import gc

        saved = gc.get_threshold()
        gc.freeze()
        gc.set_threshold(max(saved[0], 200_000), saved[1], saved[2])
        return saved

    @staticmethod
    def _gc_restore(saved) -> None:
        if saved is None:
            return
        import gc

        gc.set_threshold(*saved)
        gc.unfreeze()

    @staticmethod
    def _faults_active() -> bool:
        from ..utils.faults import injector

        return injector().active

    def _run_chunk(self, n: Node, pairs: list, faults: bool, fail_after: Optional[int]) -> None:
        """Deliver a chunk of ``(global_offset, element)`` pairs of one source: split at
        count-based barriers, then handed downstream as one ``collect_many``."""
        st = self.subtasks[id(n)][0]
        if faults:  # per-element semantics of the fault hooks
            for g, v in pairs:
                self._run_one(n, g, v, st, fail_after)
            return
        every = self.env.checkpoint_every if n is self.primary else None
        i, m = 0, len(pairs)
        while i < m:
            j = m
            if every:
                self._maybe_checkpoint(pairs[i][0])
                nb = self.next_cid * every
                j = bisect.bisect_left(pairs, nb, lo=i, key=_first)
                j = max(j, i + 1)
            sub = pairs if (i == 0 and j == m) else pairs[i:j]
            self.processed[id(n)] = sub[-1][0] + 1
            vals = [v for _, v in sub]
            self.elements_in += len(vals)
            self.records_in += len(vals) if not any(issubclass(t, RecordBatch) for t in set(map(type, vals))) else \
                sum(len(v) if isinstance(v, RecordBatch) else 1 for v in vals)
            st.out.collect_many(vals)
            i = j

    def _run_one(self, n: Node, g: int, v: Any, st: _Subtask, fail_after: Optional[int]) -> None:
        if self.env.checkpoint_every and n is self.primary:
            self._maybe_checkpoint(g)
        self.processed[id(n)] = g + 1
        self.elements_in += 1
        self.records_in += len(v) if isinstance(v, RecordBatch) else 1
        if fail_after is not None and self.elements_in > fail_after:
            raise SimulatedFailure(f"injected failure after {fail_after} records")
        if self.dist is not None:
            from ..utils.faults import injector

            injector().on_batch(self.rank, self.elements_in - 1)
        st.out.collect(v)

    def _make_inputs(self, sources: List[Node], mode: str):
        from .inputs import DeterministicInputs, LiveInputs

        if mode == "live":
            poll = 0.05
            cfg = self.env.config
            if cfg is not None and cfg.watchdog_s:
                poll = min(poll, cfg.watchdog_s / 4)
            if self.env.checkpoint_interval_ms:
                poll = min(poll, self.env.checkpoint_interval_ms / 4e3)
            return LiveInputs(sources, self.readers, self.clock, poll_s=poll)
        return DeterministicInputs(sources, self.readers)

    def run(self, job_name: str) -> JobExecutionResult:
        t0 = time.perf_counter()
        gc_saved = self._gc_tune()
        self.clock.bind_thread()
        set_current_clock(self.clock)
        cfg = self.env.config
        inputs = None
        try:
            doc = self._restored_doc()
            self._instantiate(doc)
            sources = self._open_readers(doc)
            mode = self._input_mode(sources)
            self.input_mode = mode
            self._check_checkpoint_config(sources, mode)
            inputs = self._make_inputs(sources, mode)
            if self.env.checkpoint_interval_ms and self.dist:
                from .coordinator import CheckpointCoordinator

                self.coordinator = CheckpointCoordinator(self.dist, self.env.checkpoint_interval_ms / 1e3,
                                                         inputs.inject, first_cid=self.next_cid).start()
            if self.dist and cfg is not None and cfg.watchdog_s:
                from ..utils.faults import Watchdog

                self.watchdog = Watchdog(cfg.watchdog_s, name=f"rank{self.rank}").start()
            fail_after = self.env.fail_after
            time_ckpt = bool(self.env.checkpoint_interval_ms)
            dist_hooks = self.dist is not None
            faults = fail_after is not None or (dist_hooks and self._faults_active())
            for item in inputs:
                if type(item) is Chunk:
                    self._run_chunk(item.node, item.pairs, faults, fail_after)
                elif type(item) is tuple:
                    n, g, v = item
                    self._run_one(n, g, v, self.subtasks[id(n)][0], fail_after)
                elif item.kind == "barrier":
                    self._checkpoint(item.cid)
                    self.next_cid = item.cid + 1
                elif item.kind == "error":
                    raise item.exc
                elif item.kind == "stop":  # pragma: no cover - only after end of input
                    break
                if self.watchdog is not None:
                    self.watchdog.kick()
                self.clock.fire_due()
                if time_ckpt:
                    self._time_checkpoint_due()
            self._finish_input(inputs)
        except Exception as e:  # noqa: BLE001 - any operator failure fails the job
            raise JobExecutionException(f"Job '{job_name}' failed: {type(e).__name__}: {e}") from e
        finally:
            if self.coordinator is not None:
                self.coordinator.stop()
            if inputs is not None:
                inputs.close()
            if self.watchdog is not None:
                self.watchdog.stop()
            self.clock.timers.clear()
            set_current_clock(None)
            self._gc_restore(gc_saved)
            for n in self.nodes:
                for st in self.subtasks.get(id(n), []):
                    if isinstance(st.op, (RichFunction, SinkFunction)):
                        try:
                            st.op.close()
                        except Exception:  # noqa: BLE001
                            logger.exception("close() failed")
        METRICS.inc("job.records_in", self.records_in)
        METRICS.inc("job.elements_in", self.elements_in)
        return JobExecutionResult(job_name, (time.perf_counter() - t0) * 1e3, self.records_in, self.checkpoint_paths,
                                  elements_in=self.elements_in, input_mode=getattr(self, "input_mode", None))


def _first(pair):
    return pair[0]


def _clone(op: Any) -> Any:
    """Per-subtask copy of an operator; goes through cloudpickle when available so that an
    operator that could not be shipped to a remote worker fails here, like Flink's
    ``ClosureCleaner.clean(..., checkSerializable = true)``."""
    try:
        import cloudpickle

        return cloudpickle.loads(cloudpickle.dumps(op))
    except ImportError:  # pragma: no cover
        return copy.deepcopy(op)


def ensure_serializable(obj: Any) -> Any:
    import cloudpickle

    return cloudpickle.loads(cloudpickle.dumps(obj))
