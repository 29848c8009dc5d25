"""Pipelined micro-batch scoring engine (host records → GPU → host predictions).

The reference scores one record at a time on the JVM (`S/package.scala:76-79`). Here a stream of
records is scored in micro-batches through a three-stage pipeline on HIP streams:

    H2D stream:   pinned host slice ──copy──▶ device input slot[i % depth]
    compute:      wait(H2D[i]) ▶ fused prepare + model kernel ▶ scores written by the epilogue
                  straight into pinned host memory (zero-copy) [+ optional device mirror]
    D2H stream:   only for plans without a zero-copy epilogue: device scores ──copy──▶ host

A ring of ``depth`` device input slots lets batch i+1's copy overlap batch i's kernel. Nothing in
:meth:`StreamingScorer.submit_batch` blocks the host: it returns a
:class:`~flink_jpmml_amd.api.batch.PredictionBatch` future whose buffers the kernel fills; the
only synchronisation points are reading that future and the in-flight cap (backpressure). PCIe
Gen5 (≈50+ GB/s per GPU) is the usual bound for wide fp32 records; the kernels run far below it
(see ``profiles/``).

A :class:`~flink_jpmml_amd.api.batch.SparseRecordBatch` takes the same ring without being
densified on the host: each slice's CSR arrays (``indptr`` rebased to 0, ``indices``, ``values``)
are copied into staging buffers that belong to the ring slot, ``pmml_csr_expand`` rebuilds the dense
rows in the slot on the compute stream (absent entries take ``replace_nan``, else NaN), and the plan
runs on them as on any other slot.

One :class:`DevicePipeline` (streams + input ring) is shared by every model an operator serves on
a device, so a dynamic-serving operator with 64 cached models holds one ring, not 64.

Scorers (all expose ``submit_batch(batch, replace_nan) -> PredictionBatch``):

* :class:`StreamingScorer` — device plan on the pipeline (the GPU path);
* :class:`HostScorer` — vectorised float64 oracle (``device=None`` or an explicit host fallback);
* :class:`NullScorer` — a model without a target field: every row is ``EmptyScore``.

:func:`make_scorer` picks one under the :class:`~flink_jpmml_amd.config.ScoringConfig` fallback
policy (never silently: host fallbacks are logged and counted).
"""

from __future__ import annotations

import collections
import logging
import threading
import time
from dataclasses import dataclass
from typing import Tuple, List, Optional

import numpy as np

from ..api.batch import PredictionBatch, RecordBatch, SparseRecordBatch
from ..ops.sparse import MAX_WIDTH as CSR_MAX_WIDTH
from ..utils.metrics import METRICS
from ..utils.profiling import prange

logger = logging.getLogger(__name__)


@dataclass
class StepHandle:
    n: int
    done: object  # torch.cuda.Event recorded on the D2H (or compute) stream
    score_dev: object = None
    valid_dev: object = None
    out_index: int = 0


SPLIT_COPY_MIN_BYTES = 8 << 20  # micro-batch copies below this size use one copy stream


class DevicePipeline:
    """HIP streams + the device input ring, shareable by several plans on one device. The ring
    holds ``depth`` flat fp32 slots of ``micro_batch × max_features`` (grown on demand)."""

    def __init__(self, device, micro_batch: int = 1 << 19, depth: int = 3, h2d_streams: int = 0):
        import torch

        self.device = torch.device(device)
        self.B = int(micro_batch)
        self.depth = int(depth)
        # each micro-batch copy may be split over `h2d_streams` streams (concurrent copy engines).
        # 0 = auto: the first copy calibrates 1 vs 2 streams on this box and keeps the faster —
        # measured: one box moves a whole 128 MiB micro-batch at 56 GB/s on one stream, another at
        # 34 GB/s on one and 56 GB/s split over two (profiles/r2_h2d_probe.md)
        self.auto_h2d = int(h2d_streams) <= 0
        self.h2ds = [torch.cuda.Stream(self.device) for _ in range(2 if self.auto_h2d else int(h2d_streams))]
        self.n_h2d = None if self.auto_h2d else len(self.h2ds)
        self.h2d = self.h2ds[0]
        self.comp = torch.cuda.Stream(self.device)
        self.d2h = torch.cuda.Stream(self.device)
        self.slot_elems = 0
        self.slots: List = []
        self.ev_h2d = [[torch.cuda.Event() for _ in self.h2ds] for _ in range(self.depth)]
        self.ev_comp = [torch.cuda.Event() for _ in range(self.depth)]
        self.used = [False] * self.depth
        self.next = 0
        self._dev_ptr_cache = {}
        # CSR staging of each ring slot (sparse batches): [indptr int32, indices int32, values fp32]
        self.csr: List = [None] * self.depth

    def ensure_slots(self, elems: int) -> None:
        if elems <= self.slot_elems:
            return
        import torch

        for t in self.slots:  # queued kernels / copies may still use the old ring
            t.record_stream(self.comp)
            for st in self.h2ds:
                t.record_stream(st)
        self.slots = [torch.empty(elems, dtype=torch.float32, device=self.device) for _ in range(self.depth)]
        self.slot_elems = elems

    def ensure_csr(self, slot: int, rows: int, nnz: int):
        """The CSR staging tensors of ring slot ``slot`` with room for ``rows + 1`` indptr words and
        ``nnz`` entries (grown on demand, like :meth:`ensure_slots`). The slot's events order their
        reuse: the next H2D into them waits for ``ev_comp[slot]``."""
        import torch

        cur = self.csr[slot]
        if cur is not None and cur[0].numel() >= rows + 1 and cur[1].numel() >= nnz:
            return cur
        if cur is not None:  # queued kernels / copies may still use the old staging
            for t in cur:
                t.record_stream(self.comp)
                for st in self.h2ds:
                    t.record_stream(st)
            rows, nnz = max(rows, cur[0].numel() - 1), max(nnz, cur[1].numel())
        cap = max(1024, nnz + (nnz >> 2))  # headroom: slices of one stream differ in nnz
        cur = [torch.empty(max(rows, self.B) + 1, dtype=torch.int32, device=self.device),
               torch.empty(cap, dtype=torch.int32, device=self.device),
               torch.empty(cap, dtype=torch.float32, device=self.device)]
        self.csr[slot] = cur
        return cur

    @property
    def h2d_streams_in_use(self) -> Optional[int]:
        """Copy streams this pipeline splits each micro-batch over (``None`` before the auto
        calibration ran)."""
        return self.n_h2d

    def active_h2d(self) -> List:
        """The copy streams in use (calibrated on first use in auto mode)."""
        if self.n_h2d is None:
            self.n_h2d = self._calibrate_h2d()
        return self.h2ds[: self.n_h2d]

    def _calibrate_h2d(self, mib: int = 128, reps: int = 3) -> int:
        import time

        import torch

        n = mib * (1 << 18)  # fp32 elements
        src = torch.empty(n, dtype=torch.float32, pin_memory=True)
        src.fill_(1.0)
        dst = torch.empty(n, dtype=torch.float32, device=self.device)
        best = {}
        for k in (1, 2):
            part = -(-n // k)
            ts = []
            for _ in range(reps + 1):
                torch.cuda.synchronize(self.device)
                t0 = time.perf_counter()
                for j in range(k):
                    with torch.cuda.stream(self.h2ds[j]):
                        dst[j * part:(j + 1) * part].copy_(src[j * part:(j + 1) * part], non_blocking=True)
                torch.cuda.synchronize(self.device)
                ts.append(time.perf_counter() - t0)
            best[k] = min(ts[1:])
        del src, dst
        # ties go to 2 streams: never slower on the boxes measured (56 vs 56 GB/s), 1.6x faster on
        # the single-stream-limited ones (34 vs 56 GB/s), and with N ranks calibrating at once
        # (host-memory contention) the timings are noisy — only a clear 1-stream win keeps 1
        choice = 1 if best[1] < 0.97 * best[2] else 2
        from ..utils.metrics import METRICS

        METRICS.observe("pipeline.h2d_calibration_gbps_1", mib * 1.048576e-3 / best[1])
        METRICS.observe("pipeline.h2d_calibration_gbps_2", mib * 1.048576e-3 / best[2])
        # one observation per calibrated pipeline (a histogram, not a summed counter: the BENCH line
        # reports the distribution, never "4 streams" from four pipelines choosing 1)
        METRICS.observe("pipeline.h2d_streams_chosen", float(choice))
        return choice

    def host_dev_ptr(self, t):
        from ..ops._lib import host_device_ptr

        key = (t.data_ptr(), t.numel())
        p = self._dev_ptr_cache.get(key)
        if p is None:
            p = host_device_ptr(t)
            if len(self._dev_ptr_cache) > 4096:
                self._dev_ptr_cache.clear()
            self._dev_ptr_cache[key] = p
        return p


def _pin(X):
    """Host matrix → contiguous float32 pinned tensor (one host copy)."""
    import torch

    if isinstance(X, torch.Tensor):
        src = X.to(torch.float32).contiguous()
    else:
        src = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    out = torch.empty(src.shape, dtype=torch.float32, pin_memory=True)
    out.copy_(src)
    return out


def _pin_as(a: np.ndarray, dtype):
    """1-D host array → pinned tensor of ``dtype`` (one host copy)."""
    import torch

    src = torch.from_numpy(np.ascontiguousarray(a))
    out = torch.empty(src.shape, dtype=dtype, pin_memory=True)
    out.copy_(src)
    return out


@dataclass
class _CsrSource:
    """A sparse batch staged for the H2D ring (see :meth:`StreamingScorer._stage_csr`)."""
    batch: object
    indptr: np.ndarray  # the batch's own row starts (host)
    rebased: object  # pinned int32: every micro-batch slice's indptr rebased to 0
    indices: object  # pinned int32 [>= nnz]
    values: object  # pinned fp32 [>= nnz]
    fill: float


class StreamingScorer:
    kind = "device"

    def __init__(self, plan, micro_batch: int = 131072, depth: int = 3, max_rows: Optional[int] = None,
                 out_buffers: int = 2, direct_host_output: bool = True, keep_device_output: bool = True,
                 h2d_streams: int = 0, pipeline: Optional[DevicePipeline] = None, max_inflight: int = 4,
                 graph_max_rows: int = 0):
        self.plan = plan
        self.device = plan.device
        self.F = plan.n_features
        self.pipe = pipeline if pipeline is not None else DevicePipeline(self.device, micro_batch, depth, h2d_streams)
        self.B = self.pipe.B
        self.depth = self.pipe.depth
        self.h2ds, self.h2d, self.comp, self.d2h = self.pipe.h2ds, self.pipe.h2d, self.pipe.comp, self.pipe.d2h
        self.max_rows = max_rows or self.B
        # step output buffers of the step API (bench engine mode), used round-robin
        self.n_out = int(out_buffers)
        self._outs = None
        self._out_free: List[Optional[object]] = [None] * self.n_out
        self._out_i = 0
        self.batch_times_ms: List[float] = []
        # zero-copy sink: the kernel epilogue writes scores straight into pinned host memory over
        # PCIe (no D2H copy commands: small D2H copies were measured to stall the H2D stream)
        self.direct = bool(direct_host_output) and getattr(plan, "supports_direct", False)
        self.keep_device = keep_device_output
        self.max_inflight = int(max_inflight)
        self._inflight: "collections.deque" = collections.deque()
        self.rows_submitted = 0
        # Output-field plans by top_k, lowered on first use under the config's policy (make_scorer)
        self._out_plans: dict = {}
        self._out_lock = threading.Lock()
        self.fallback = "warn"
        self.lowering_opts: dict = {}
        self.reason_codes = False  # ScoringConfig.reason_codes: passed to output_plan only
        self.entity_ranks = False  # ScoringConfig.entity_ranks: likewise
        self.knn_classes = False  # ScoringConfig.knn_classes: likewise
        self.svm_classes = False  # ScoringConfig.svm_classes: likewise
        self._row_state = None  # score_row's persistent buffers
        self._row_lock = threading.Lock()  # ...shared by every caller of score_row
        from ..ops import _lib

        self._lib = _lib.load()
        # multi-kernel plans: small micro-batches as one HIP-graph replay (runtime/graphs.py)
        self._graphs = None
        if graph_max_rows > 0 and getattr(plan, "graph_small_batches", False):
            from .graphs import GraphLauncher

            self._graphs = GraphLauncher(plan, max_rows=graph_max_rows)

    # ------------------------------------------------------------------ step API (bench engine mode)
    def _alloc_out(self, n: int):
        import torch

        return (torch.empty(n, dtype=torch.float32, device=self.device),
                torch.empty(n, dtype=torch.uint8, device=self.device))

    @property
    def score_dev(self):
        self.ensure_capacity(0)
        return self._outs[(self._out_i - 1) % self.n_out][0]

    @property
    def valid_dev(self):
        self.ensure_capacity(0)
        return self._outs[(self._out_i - 1) % self.n_out][1]

    def ensure_capacity(self, n: int) -> None:
        if n > self.max_rows or self._outs is None:
            if self._outs is not None:
                # kernels already queued on the compute stream may still write the old buffers:
                # the caching allocator recycles them only once that stream's queued work is done
                for pair in self._outs:
                    for t in pair:
                        t.record_stream(self.comp)
            self.max_rows = max(n, self.max_rows)
            self._outs = [self._alloc_out(self.max_rows) for _ in range(self.n_out)]
            self._out_free = [None] * self.n_out

    def _slot(self, m: int):
        p = self.pipe
        p.ensure_slots(p.B * max(self.F, 1))
        slot = p.next
        p.next = (slot + 1) % p.depth
        return slot, p.slots[slot][: m * self.F].view(m, self.F)

    def _enqueue(self, X_src, s: int, e: int, out_score, out_valid, kw) -> None:
        """H2D rows ``[s, e)`` of ``X_src`` into the next ring slot (or use them in place when they
        are on the device already) and launch the plan on the compute stream."""
        import torch

        p = self.pipe
        m = e - s
        if X_src.is_cuda:
            xs, slot = X_src[s:e], None
        else:
            slot, xs = self._slot(m)
            h2ds = p.active_h2d()
            if len(h2ds) > 1 and m * self.F * 4 < SPLIT_COPY_MIN_BYTES:
                h2ds = h2ds[:1]  # a small copy gains nothing from a second copy engine, only API calls
            part = -(-m // len(h2ds))
            raw = X_src.is_contiguous() and X_src.dtype == torch.float32
            if raw:  # hipMemcpyAsync straight from the pinned rows: no torch stream contexts per copy
                rowb = self.F * 4
                src0, dst0 = X_src.data_ptr() + s * rowb, xs.data_ptr()
            for j, st in enumerate(h2ds):
                if p.used[slot]:
                    st.wait_event(p.ev_comp[slot])  # kernel finished reading this slot
                a, b = j * part, min(m, (j + 1) * part)
                if a < b:
                    if raw:
                        rc = self._lib.pmml_memcpy_async(dst0 + a * rowb, src0 + a * rowb, (b - a) * rowb, 1,
                                                             st.cuda_stream)
                        if rc != 0:
                            raise RuntimeError(f"hipMemcpyAsync H2D failed ({rc})")
                    else:
                        with torch.cuda.stream(st):
                            xs[a:b].copy_(X_src[s + a:s + b], non_blocking=True)
                p.ev_h2d[slot][j].record(st)
            for ev in p.ev_h2d[slot][: len(h2ds)]:
                p.comp.wait_event(ev)
        self._launch(xs, slot, m, out_score, out_valid, kw)

    def _launch(self, xs, slot, m: int, out_score, out_valid, kw) -> None:
        """The plan (or its graph) over the ``m`` device rows ``xs`` on the compute stream; then ring
        slot ``slot`` (if any) is marked busy until that work is done."""
        p = self.pipe
        g = self._graphs
        if kw.get("outputs") is not None:  # the Output fields route: the output plan, never a graph
            kw = dict(kw)
            kw.pop("plan").launch(xs, out_score, out_valid, stream=p.comp, **kw)
        elif g is not None and g.applies(m, kw):
            g.launch(xs, out_score, out_valid, stream=p.comp, **kw)
        else:
            self.plan.launch(xs, out_score, out_valid, stream=p.comp, **kw)
        if slot is not None:
            p.ev_comp[slot].record(p.comp)
            p.used[slot] = True

    def submit(self, X_host, score_host=None, valid_host=None, offset: int = 0) -> StepHandle:
        """Enqueue scoring of a pinned host matrix ``X_host`` ([n, F] float32 tensor). Scores land in
        this step's device output buffer (``handle.score_dev``) and, if given, in the pinned host
        outputs. Returns immediately."""
        import torch

        n = int(X_host.shape[0])
        self.ensure_capacity(offset + n)
        oi = self._out_i
        self._out_i = (oi + 1) % self.n_out
        score_dev, valid_dev = self._outs[oi]
        if self._out_free[oi] is not None:
            self.comp.wait_event(self._out_free[oi])  # WAR: the step that last used this buffer
        hs = hv = None
        if self.direct and score_host is not None and valid_host is not None:
            hs, hv = self.pipe.host_dev_ptr(score_host), self.pipe.host_dev_ptr(valid_host)
            if hs is None or hv is None:
                hs = hv = None
        for s in range(0, n, self.B):
            e = min(n, s + self.B)
            if hs is not None:
                kw = {}
                if self.keep_device:
                    kw = dict(score2=score_dev[offset + s: offset + e], valid2=valid_dev[offset + s: offset + e])
                self._enqueue(X_host, s, e, hs + 4 * s, hv + s, kw)
            else:
                self._enqueue(X_host, s, e, score_dev[offset + s: offset + e], valid_dev[offset + s: offset + e], {})
                if score_host is not None:
                    ev = torch.cuda.Event()
                    ev.record(self.comp)
                    with torch.cuda.stream(self.d2h):
                        self.d2h.wait_event(ev)
                        score_host[s:e].copy_(score_dev[offset + s: offset + e], non_blocking=True)
                        if valid_host is not None:
                            valid_host[s:e].copy_(valid_dev[offset + s: offset + e], non_blocking=True)
        done = torch.cuda.Event()
        if score_host is not None and hs is None:
            done.record(self.d2h)
        else:
            done.record(self.comp)
        self._out_free[oi] = done
        h = StepHandle(n, done)
        h.score_dev = score_dev[offset: offset + n]
        h.valid_dev = valid_dev[offset: offset + n]
        h.out_index = oi
        return h

    def mark_consumed(self, handle: StepHandle, stream) -> None:
        """Declare that ``stream`` also reads this step's device outputs (e.g. an all-gather): the
        step that next reuses the buffer waits for it."""
        import torch

        ev = torch.cuda.Event()
        ev.record(stream)
        prev = self._out_free[handle.out_index]
        if prev is not None:
            stream.wait_event(prev)
            ev = torch.cuda.Event()
            ev.record(stream)
        self._out_free[handle.out_index] = ev

    def join(self, stream=None) -> None:
        """Make ``stream`` (default: current) wait for all work submitted so far (no host sync)."""
        import torch

        s = stream or torch.cuda.current_stream(self.device)
        for st in (*self.h2ds, self.comp, self.d2h):
            ev = torch.cuda.Event()
            ev.record(st)
            s.wait_event(ev)

    @staticmethod
    def wait(handle: StepHandle) -> None:
        handle.done.synchronize()

    # ------------------------------------------------------------------ future API (DSL)
    def _throttle(self) -> None:
        # entries: (completion event, source rows): raw hipMemcpyAsync copies do not register with
        # torch's pinned-memory allocator, so the rows stay referenced until their work is done
        while len(self._inflight) >= self.max_inflight:
            self._inflight.popleft()[0].synchronize()
        while self._inflight and self._inflight[0][0].query():
            self._inflight.popleft()

    def _output_plan(self, top_k: int):
        """The model's :class:`~flink_jpmml_amd.runtime.outputs.OutputPlan`, lowered on first use;
        a :class:`HostScorer` instead when it does not lower and the fallback policy allows."""
        op = self._out_plans.get(top_k)
        if op is not None:
            return op
        with self._out_lock:  # one lowering, one warning and one fallback count per top_k
            op = self._out_plans.get(top_k)
            if op is None:
                op = self._out_plans[top_k] = self._lower_outputs(top_k)
        return op

    def _lower_outputs(self, top_k: int):
        """:meth:`_output_plan`'s first use (under its lock): lower, or fall back as the policy says."""
        from .plans import NotLowerable

        compiled = getattr(self.plan, "compiled", None)
        if compiled is None or not hasattr(compiled, "output_plan"):
            from ..api.exceptions import UnsupportedFeatureException

            raise UnsupportedFeatureException(
                "Output fields need the PMML document: this scorer's plan arrived by replication "
                "without it (bind the model from its document on this rank)")
        try:
            return compiled.output_plan(self.device, top_k=top_k, reason_codes=self.reason_codes,
                                        entity_ranks=self.entity_ranks, knn_classes=self.knn_classes,
                                        svm_classes=self.svm_classes, **self.lowering_opts)
        except NotLowerable as e:
            if self.fallback == "error":
                raise
            METRICS.inc("scoring.host_fallback_outputs")
            if self.fallback == "warn":
                logger.warning("Output fields of model %r cannot run on %s (%s): computing them on the "
                               "host oracle (set fallback='error' to refuse)", compiled.model_name, self.device, e)
            return HostScorer(compiled, reason=str(e))

    def submit_batch(self, batch: RecordBatch, replace_nan: Optional[float] = None,
                     keep_device: bool = False, outputs: bool = False, top_k: int = 0) -> PredictionBatch:
        """Enqueue a whole RecordBatch; returns its :class:`PredictionBatch` future immediately.

        ``X`` may be pinned host memory (copied in ``micro_batch`` slices on the H2D stream),
        pageable host memory (staged through one pinned copy) or device memory (scored in place).
        ``keep_device`` additionally keeps ``[n]`` device mirrors of the outputs
        (``PredictionBatch.device_out``, for an all-gather sink). ``outputs`` also computes the
        model's ``<Output>`` fields and the ``top_k`` classes (``PredictionBatch.outputs``): the
        output plan writes device buffers, one D2H copy brings scores, validity and the output
        matrix back (the zero-copy host sink is not used on this route)."""
        import torch

        n = len(batch)
        if n == 0:
            return PredictionBatch.empty(0)
        if batch.n_features != self.F:
            raise ValueError(f"batch has {batch.n_features} features, model expects {self.F}")
        op = None
        if outputs:
            op = self._output_plan(int(top_k))
            if isinstance(op, HostScorer):
                return op.submit_batch(batch, replace_nan, outputs=True, top_k=top_k)
        if isinstance(batch, SparseRecordBatch) and self.F <= CSR_MAX_WIDTH:
            # CSR over PCIe, expanded on the device; never touches batch.X (the host densification)
            return self._submit(batch, self._stage_csr(batch, replace_nan), self._enqueue_csr, keep_device, op)
        X = batch.X
        if replace_nan is not None:  # sparse-absent entries only (host side: rare path)
            Xn = np.array(batch.numpy(), dtype=np.float32, copy=True)
            Xn[batch.absent if batch.absent is not None else np.isnan(Xn)] = replace_nan
            X = Xn
        with prange("score.stage"):
            if not isinstance(X, torch.Tensor):
                X = _pin(X)
            elif X.is_cuda:
                if X.dtype != torch.float32 or not X.is_contiguous():
                    X = X.to(torch.float32).contiguous()
                # device-resident input: the kernels on the compute stream must see the producer's
                # writes (its ready event, else its current stream), and the allocator must not
                # recycle X while they read
                if getattr(batch, "ready", None) is not None:
                    self.comp.wait_event(batch.ready)
                else:
                    self.comp.wait_stream(torch.cuda.current_stream(self.device))
                X.record_stream(self.comp)
            elif not X.is_pinned() or X.dtype != torch.float32 or not X.is_contiguous():
                X = _pin(X)
        return self._submit(batch, X, self._enqueue, keep_device, op)

    def _submit(self, batch: RecordBatch, X, enqueue, keep_device: bool, out_plan=None) -> PredictionBatch:
        """Output buffers, the ``micro_batch`` slices of the staged source ``X`` through
        ``enqueue`` (:meth:`_enqueue` for a matrix, :meth:`_enqueue_csr` for a CSR source) and the
        future over them. With ``out_plan`` every slice runs the output plan into device buffers
        and the ``[n, width]`` output matrix comes back with the scores."""
        import torch

        n = len(batch)
        self._throttle()
        score_h = torch.empty(n, dtype=torch.float32, pin_memory=True)
        valid_h = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        dev_out = None
        hs = hv = None
        out_h = out_d = None
        if self.direct and out_plan is None:
            hs, hv = self.pipe.host_dev_ptr(score_h), self.pipe.host_dev_ptr(valid_h)
            if hs is None or hv is None:
                hs = hv = None
        if keep_device or hs is None:
            with torch.cuda.stream(self.comp):
                dev_out = (torch.empty(n, dtype=torch.float32, device=self.device),
                           torch.empty(n, dtype=torch.uint8, device=self.device))
        if out_plan is not None:
            out_h = torch.empty((n, out_plan.width), dtype=torch.float32, pin_memory=True)
            with torch.cuda.stream(self.comp):
                out_d = torch.empty((n, out_plan.width), dtype=torch.float32, device=self.device)
        with prange("score.enqueue"):
            for s in range(0, n, self.B):
                e = min(n, s + self.B)
                if hs is not None:
                    kw = dict(score2=dev_out[0][s:e], valid2=dev_out[1][s:e]) if dev_out is not None else {}
                    enqueue(X, s, e, hs + 4 * s, hv + s, kw)
                elif out_plan is not None:
                    enqueue(X, s, e, dev_out[0][s:e], dev_out[1][s:e], dict(outputs=out_d[s:e], plan=out_plan))
                else:
                    enqueue(X, s, e, dev_out[0][s:e], dev_out[1][s:e], {})
            done = torch.cuda.Event()
            if hs is None:
                ev = torch.cuda.Event()
                ev.record(self.comp)
                with torch.cuda.stream(self.d2h):
                    self.d2h.wait_event(ev)
                    score_h.copy_(dev_out[0], non_blocking=True)
                    valid_h.copy_(dev_out[1], non_blocking=True)
                    if out_d is not None:
                        out_h.copy_(out_d, non_blocking=True)
                        out_d.record_stream(self.d2h)
                    for t in dev_out:
                        t.record_stream(self.d2h)
                done.record(self.d2h)
            else:
                done.record(self.comp)
        self._inflight.append((done, X))
        self.rows_submitted += n
        METRICS.inc("scoring.rows_device", n)
        METRICS.inc("scoring.batches_device")
        outputs = None
        if out_plan is not None:
            from ..api.batch import BatchOutputs

            names, k, schema, cats = out_plan.names, out_plan.top_k, out_plan.compiled.schema, out_plan.categories
            outputs = lambda: BatchOutputs.from_wide(names, out_h.numpy(), k, schema, cats)  # noqa: E731
        return PredictionBatch(n, score_h, valid_h, done, owner=(X, dev_out, out_d), on_done=_observe_latency,
                               device_out=dev_out, row_ok=batch.size_ok(), outputs=outputs)

    # ------------------------------------------------------------------ sparse (CSR) batches
    def _stage_csr(self, batch: "SparseRecordBatch", replace_nan: Optional[float]) -> "_CsrSource":
        """The pinned source of a sparse batch: its own arrays when they are pinned, else one
        pinned copy of each (as dense input is staged), plus the per-slice ``indptr`` rebased to 0
        in one pinned int32 array (slice ``j`` at ``j * (B + 1)``)."""
        import torch

        n, B, nnz = len(batch), self.B, batch.nnz
        if nnz > len(batch.indices) or nnz > len(batch.values):
            raise ValueError(f"sparse batch announces {nnz} entries, its arrays hold fewer")
        with prange("score.stage"):
            pinned = batch._pinned
            if pinned is not None:
                indices_t, values_t = pinned[1], pinned[2]
            else:
                indices_t = _pin_as(batch.indices[:nnz], torch.int32)
                values_t = _pin_as(batch.values[:nnz], torch.float32)
            n_slices = -(-n // B)
            rebased = torch.empty(n + n_slices, dtype=torch.int32, pin_memory=True)
            rb, ip = rebased.numpy(), batch.indptr
            for j in range(n_slices):
                s, e = j * B, min(n, (j + 1) * B)
                np.subtract(ip[s:e + 1], ip[s], out=rb[s + j:e + j + 1], casting="unsafe")
        fill = float("nan") if replace_nan is None else float(replace_nan)
        METRICS.inc("scoring.rows_sparse_device", n)
        METRICS.inc("scoring.h2d_bytes_sparse", 4 * (n + n_slices) + 8 * nnz)
        # `batch` rides along: the arrays its pinned tensors view stay alive until the work is done
        return _CsrSource(batch, ip, rebased, indices_t, values_t, fill)

    def _enqueue_csr(self, src: "_CsrSource", s: int, e: int, out_score, out_valid, kw) -> None:
        """H2D the CSR slice of rows ``[s, e)`` into the staging of the next ring slot, expand it
        into the slot's dense rows on the compute stream, then launch the plan as :meth:`_enqueue`
        does. The slot's events cover the staging: the next H2D into it waits for the expand
        kernel and the plan that read it."""
        from ..ops.sparse import csr_expand

        p = self.pipe
        m = e - s
        k0, k1 = int(src.indptr[s]), int(src.indptr[e])
        nnz = k1 - k0
        if nnz < 0 or k0 < 0 or k1 > src.indices.numel():
            raise ValueError(f"sparse batch: indptr[{s}:{e + 1}] = [{k0}, {k1}] is no range of its entries")
        slot, xs = self._slot(m)
        ip_d, idx_d, val_d = p.ensure_csr(slot, m, nnz)
        j = s // self.B
        h2ds = p.active_h2d()
        if len(h2ds) > 1 and nnz * 8 < SPLIT_COPY_MIN_BYTES:
            h2ds = h2ds[:1]
        # one copy engine takes indptr + indices, a second (large slices only) the values
        copies = [(ip_d.data_ptr(), src.rebased.data_ptr() + 4 * (s + j), 4 * (m + 1), 0),
                  (idx_d.data_ptr(), src.indices.data_ptr() + 4 * k0, 4 * nnz, 0),
                  (val_d.data_ptr(), src.values.data_ptr() + 4 * k0, 4 * nnz, len(h2ds) - 1)]
        for i, st in enumerate(h2ds):
            if p.used[slot]:
                st.wait_event(p.ev_comp[slot])  # expand + plan finished reading this slot's staging
            for dst, host, nbytes, lane in copies:
                if lane == i and nbytes:
                    rc = self._lib.pmml_memcpy_async(dst, host, nbytes, 1, st.cuda_stream)
                    if rc != 0:
                        raise RuntimeError(f"hipMemcpyAsync H2D failed ({rc})")
            p.ev_h2d[slot][i].record(st)
        for ev in p.ev_h2d[slot][: len(h2ds)]:
            p.comp.wait_event(ev)
        csr_expand(ip_d, idx_d, val_d, xs, nnz, src.fill, stream=p.comp)
        self._launch(xs, slot, m, out_score, out_valid, kw)

    def score_row(self, x: np.ndarray) -> Tuple[float, bool]:
        """One record (``[F]`` values, NaN = missing) through the plan, synchronously: the
        reference's per-record call pattern (`S/package.scala:76-82`) on the device. Persistent
        pinned staging and output buffers, one H2D copy, one launch on the compute stream (after
        whatever batches are queued there), the scores written straight into host-mapped memory
        when the plan's epilogue can (else one D2H copy), one stream sync — no per-call tensor
        allocation. Same kernels and row semantics as a 1-row :meth:`submit_batch`."""
        with self._row_lock:  # one set of staging buffers: concurrent callers take turns
            return self._score_row(x)

    def _score_row(self, x: np.ndarray) -> Tuple[float, bool]:
        import torch

        from ..ops._lib import check

        st = self._row_state
        if st is None:
            F = max(1, self.F)
            xh = torch.empty(F, dtype=torch.float32, pin_memory=True)
            oh = torch.empty(8, dtype=torch.float32, pin_memory=True)  # [score, valid bytes...]
            xd = torch.empty((1, F), dtype=torch.float32, device=self.device)
            sd = torch.empty(1, dtype=torch.float32, device=self.device)
            vd = torch.empty(1, dtype=torch.uint8, device=self.device)
            hs = hv = None
            if self.direct:
                base = self.pipe.host_dev_ptr(oh)
                if base is not None:
                    hs, hv = base, base + 4
            st = self._row_state = dict(xh=xh, xh_np=xh.numpy(), oh=oh, oh_np=oh.numpy(), xd=xd, sd=sd, vd=vd,
                                        hs=hs, hv=hv)
        st["xh_np"][: self.F] = x
        cs = self.comp.cuda_stream
        check(self._lib.pmml_memcpy_async(st["xd"].data_ptr(), st["xh"].data_ptr(), self.F * 4, 1, cs), "row H2D")
        g = self._graphs
        run = st.get("run", False)
        if run is False:  # the plan's prepared launch over these fixed buffers, when it has one
            rl = getattr(self.plan, "row_launcher", None)
            run = st["run"] = rl(st["xd"], st["hs"], st["hv"]) if (rl is not None and st["hs"] is not None) else None
        if run is not None:
            run(self.comp)
        elif st["hs"] is not None:
            self.plan.launch(st["xd"], st["hs"], st["hv"], stream=self.comp)
        else:
            if g is not None and g.applies(1, {}):
                g.launch(st["xd"], st["sd"], st["vd"], stream=self.comp)
            else:
                self.plan.launch(st["xd"], st["sd"], st["vd"], stream=self.comp)
            oh = st["oh"].data_ptr()
            check(self._lib.pmml_memcpy_async(oh, st["sd"].data_ptr(), 4, 2, cs), "row D2H")
            check(self._lib.pmml_memcpy_async(oh + 4, st["vd"].data_ptr(), 1, 2, cs), "row D2H")
        self.comp.synchronize()
        o = st["oh_np"]
        valid = bool(o[1:2].view(np.uint8)[0])
        METRICS.inc("scoring.rows_device")
        return float(o[0]), valid

    def score_numpy(self, X: np.ndarray) -> tuple:
        """Blocking convenience: score a host numpy matrix, return numpy ``(score, valid)``."""
        t0 = time.perf_counter()
        pb = self.submit_batch(RecordBatch(np.asarray(X, dtype=np.float32)))
        s, v = pb.scores.copy(), pb.valid.copy()
        self.batch_times_ms.append((time.perf_counter() - t0) * 1e3)
        return s, v

    def drain(self) -> None:
        while self._inflight:
            self._inflight.popleft()[0].synchronize()


def _observe_latency(pb: PredictionBatch) -> None:
    METRICS.observe("scoring.batch_latency_ms", (pb.completed - pb.submitted) * 1e3)


class HostScorer:
    """Vectorised float64 oracle with the scorer interface (host path / explicit fallback)."""

    kind = "host"
    direct = False

    def __init__(self, compiled, reason: Optional[str] = None):
        self.compiled = compiled
        self.reason = reason
        self.F = compiled.n_features

    def submit_batch(self, batch: RecordBatch, replace_nan: Optional[float] = None,
                     keep_device: bool = False, outputs: bool = False, top_k: int = 0) -> PredictionBatch:
        n = len(batch)
        if n == 0:
            return PredictionBatch.empty(0)
        if batch.n_features != self.F:
            raise ValueError(f"batch has {batch.n_features} features, model expects {self.F}")
        t0 = time.perf_counter()
        outs = None
        with prange("score.host"):
            if outputs:
                from .outputs import host_batch_outputs

                s, v, outs = host_batch_outputs(self.compiled, batch.numpy(), replace_nan, batch.absent, top_k)
            else:
                s, v = self.compiled.score_matrix_oracle(batch.numpy(), replace_nan, batch.absent)
        METRICS.inc("scoring.rows_host", n)
        if self.reason is not None:
            METRICS.inc("scoring.host_fallback_rows", n)
        METRICS.observe("scoring.batch_latency_ms", (time.perf_counter() - t0) * 1e3)
        return PredictionBatch(n, s.astype(np.float32), v, row_ok=batch.size_ok(), outputs=outs)

    def drain(self) -> None:
        pass


class NullScorer:
    """A model without a named target field: the reference extracts nothing and every record is
    ``EmptyScore`` (`S/api/PmmlModel.scala:167-174`). ``rule_plan``: the output plan of an
    AssociationModel under ``ScoringConfig.association_rules`` (:func:`make_scorer` lowers it); with
    it the Output fields of a batch come from the device, without it from the host oracle."""

    kind = "null"
    direct = False

    def __init__(self, n_features: int, compiled=None, rule_plan=None):
        self.F = n_features
        self.compiled = compiled
        self.rule_plan = rule_plan
        self.device = rule_plan.device if rule_plan is not None else None

    def _submit_rules(self, batch: RecordBatch, replace_nan: Optional[float]) -> PredictionBatch:
        """The batch through the rule plan: one launch, one copy of the output matrix back."""
        from ..api.batch import BatchOutputs

        plan = self.rule_plan
        if isinstance(batch, SparseRecordBatch) and self.F <= CSR_MAX_WIDTH:
            _, _, wide = plan.score_csr_outputs(batch, replace_nan)
        else:
            _, _, wide = plan.score_outputs(batch.X, replace_nan, absent=batch.absent)
        n = len(batch)
        outs = BatchOutputs.from_wide(plan.names, wide.cpu().numpy(), 0, plan.compiled.schema, None)
        METRICS.inc("scoring.rows_device", n)
        METRICS.inc("scoring.batches_device")
        return PredictionBatch(n, np.full(n, np.nan, dtype=np.float32), np.zeros(n, dtype=bool),
                               row_ok=batch.size_ok(), outputs=outs)

    def submit_batch(self, batch: RecordBatch, replace_nan: Optional[float] = None,
                     keep_device: bool = False, outputs: bool = False, top_k: int = 0) -> PredictionBatch:
        METRICS.inc("scoring.empty_score.no_target", len(batch))
        if outputs and self.rule_plan is not None and not top_k and len(batch) and batch.n_features == self.F:
            return self._submit_rules(batch, replace_nan)
        if outputs and self.compiled is not None and len(batch) and batch.n_features == self.F:
            from .outputs import host_batch_outputs  # every score is empty, the Output fields are not

            s, v, outs = host_batch_outputs(self.compiled, batch.numpy(), replace_nan, batch.absent, top_k)
            return PredictionBatch(len(batch), s.astype(np.float32), v, row_ok=batch.size_ok(), outputs=outs)
        return PredictionBatch.empty(len(batch))

    def drain(self) -> None:
        pass


def _set_host_threads(n: int) -> None:
    """Worker threads of the native host tree walk (process-wide)."""
    from ..native import fastpath

    fp = fastpath()
    if fp is not None and hasattr(fp, "set_walk_threads"):
        fp.set_walk_threads(int(n))


def _rule_plan(compiled, device, cfg):
    """The output plan of an AssociationModel under ``cfg.association_rules`` on ``device``, or None:
    switch off, no device, another model, or a document the rule kernel cannot take and a fallback
    policy that allows the host path (``error`` fails the load instead)."""
    from ..models.association import AssociationEvaluator
    from .plans import NotLowerable

    if device is None or not cfg.association_rules or not isinstance(compiled.evaluator, AssociationEvaluator):
        return None
    try:
        with prange("model.lower"):
            return compiled.output_plan(device, association_rules=True, **cfg.lowering_opts())
    except NotLowerable as e:
        if cfg.fallback == "error":
            from ..api.exceptions import ModelLoadingException

            raise ModelLoadingException(f"Output fields of model {compiled.model_name!r} are not lowerable to "
                                        f"{device}: {e}", e) from e
        METRICS.inc("scoring.host_fallback_outputs")
        if cfg.fallback == "warn":
            logger.warning("Output fields of model %r cannot run on %s (%s): computing them on the "
                           "host oracle (set fallback='error' to refuse)", compiled.model_name, device, e)
        return None


def make_scorer(compiled, device, config=None, pipeline: Optional[DevicePipeline] = None, plan=None,
                lower_error: Optional[str] = None):
    """The scorer for ``compiled`` on ``device`` under ``config``'s fallback policy.

    * no target field → :class:`NullScorer` (for an AssociationModel under ``config.association_rules``
      on a device: with the output plan that ranks its rules, lowered here under the same policy);
    * ``device is None`` → :class:`HostScorer`;
    * otherwise the device plan; a model the device path cannot lower goes to the host oracle with
      a WARNING + ``scoring.host_fallback_models`` (``fallback="warn"``), only counted
      (``"host"``), or fails the load (``"error"``). Device *runtime* errors always propagate."""
    from ..config import ScoringConfig
    from .plans import NotLowerable

    cfg = config or ScoringConfig()
    if not compiled.target_fields:
        return NullScorer(compiled.n_features, compiled, _rule_plan(compiled, device, cfg))
    if cfg.host_threads:
        _set_host_threads(cfg.host_threads)
    if device is None:
        return HostScorer(compiled)
    if plan is None:
        try:
            if lower_error is not None:  # the leader rank already failed to lower this model
                raise NotLowerable(lower_error)
            with prange("model.lower"):
                plan = compiled.plan(device, **cfg.lowering_opts())
        except NotLowerable as e:
            if cfg.fallback == "error":
                from ..api.exceptions import ModelLoadingException

                raise ModelLoadingException(f"model {compiled.model_name!r} is not lowerable to {device}: {e}",
                                            e) from e
            METRICS.inc("scoring.host_fallback_models")
            if cfg.fallback == "warn":
                logger.warning("model %r cannot run on %s (%s): scoring it on the host oracle "
                               "(set fallback='error' to refuse)", compiled.model_name, device, e)
            return HostScorer(compiled, reason=str(e))
    if pipeline is None:
        pipeline = DevicePipeline(plan.device, cfg.micro_batch, cfg.pipeline_depth, cfg.h2d_streams)
    scorer = StreamingScorer(plan, pipeline=pipeline, max_inflight=cfg.max_inflight, graph_max_rows=cfg.graph_max_rows)
    scorer.fallback, scorer.lowering_opts = cfg.fallback, dict(cfg.lowering_opts())
    scorer.reason_codes = bool(cfg.reason_codes)
    scorer.entity_ranks = bool(cfg.entity_ranks)
    scorer.knn_classes = bool(cfg.knn_classes)
    scorer.svm_classes = bool(cfg.svm_classes)
    return scorer


__all__ = ["DevicePipeline", "HostScorer", "NullScorer", "StepHandle", "StreamingScorer", "make_scorer"]
