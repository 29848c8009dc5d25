#!/usr/bin/env python3
"""Sparse (CSR) against dense record batches, end to end and per kernel, on one GBDT.

For ``--features`` wide records of which a fraction ``--density`` is stored, ``--rows`` per batch:

* end-to-end rows/s of the same records sent as dense ``RecordBatch`` (absent = NaN) and as
  ``SparseRecordBatch`` through ``quick_evaluate`` (pinned host memory -> scores on the host);
* the ``pmml_csr_expand`` kernel's time on one micro-batch slice;
* a plain device fill (``tensor.fill_``) of the same ``[m, F]`` tensor -- the floor for writing
  ``m * F * 4`` bytes -- and the model kernel's time on that tensor.

Prints one JSON line. ``--mode dense`` needs no sparse support (to measure an older checkout).

python scripts/sparse_bench.py --features 512 --density 0.05 --rows 1000000 --trees 100 --depth 6
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_csr(rows: int, F: int, density: float, seed: int):
    """Random CSR rows: each entry stored with probability ``density`` (fp32 values)."""
    rng = np.random.default_rng(seed)
    counts, idx = [], []
    for r0 in range(0, rows, 1 << 16):
        mask = rng.random((min(1 << 16, rows - r0), F), dtype=np.float32) < density
        counts.append(mask.sum(axis=1))
        idx.append(np.nonzero(mask)[1].astype(np.int32))
    indptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(np.concatenate(counts), out=indptr[1:])
    indices = np.concatenate(idx)
    values = rng.standard_normal(indices.size, dtype=np.float32)
    return indptr, indices, values


def pinned_like(a):
    import torch

    t = torch.empty(a.shape, dtype=torch.from_numpy(a[:0]).dtype, pin_memory=True)
    t.numpy()[...] = a
    return t


def dense_pinned(indptr, indices, values, rows: int, F: int):
    import torch

    X = torch.empty((rows, F), dtype=torch.float32, pin_memory=True)
    Xn = X.numpy()
    Xn.fill(np.nan)
    Xn[np.repeat(np.arange(rows), np.diff(indptr)), indices] = values
    return X


def run_stream(batch, path: str, device, copies: int, micro_batch: int):
    """Wall seconds of ``copies`` copies of ``batch`` through ``quick_evaluate`` until every score
    is on the host, and the last PredictionBatch."""
    from flink_jpmml_amd import ModelReader
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.stream import StreamExecutionEnvironment

    cfg = ScoringConfig(device=device, micro_batch=micro_batch, fallback="error")
    t0 = time.perf_counter()
    env = StreamExecutionEnvironment(config=cfg)
    out = env.from_batches([batch] * copies).quick_evaluate(ModelReader(path)).collect()
    for p, _ in out:
        p.wait()
    return time.perf_counter() - t0, out[-1][0]


def end_to_end(batch, path: str, device, warmup: int, reps: int, micro_batch: int):
    """Steady-state rows/s through ``quick_evaluate``: a job of ``warmup + reps`` copies of
    ``batch`` against a job of ``warmup`` copies -- model load, lowering, ring allocation and H2D
    calibration are in both and cancel. A first job (discarded) takes the process's one-time costs."""
    run_stream(batch, path, device, warmup, micro_batch)
    t_short, _ = run_stream(batch, path, device, warmup, micro_batch)
    t_long, pb = run_stream(batch, path, device, warmup + reps, micro_batch)
    if t_long <= t_short:
        raise SystemExit(f"{reps} x {len(batch)} rows vanish in the timing noise ({t_short:.3f} s against "
                         f"{t_long:.3f} s): raise --rows or --reps")
    return reps * len(batch) / (t_long - t_short), pb


def event_ms(fn, stream_sync, reps: int):
    import torch

    fn()
    stream_sync()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro-batch", type=int, default=1 << 19)
    ap.add_argument("--mode", choices=["both", "dense", "sparse"], default="both")
    ap.add_argument("--no-kernels", action="store_true", help="skip the kernel-only timings")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.bench.synth import gbdt_pmml

    F, rows = args.features, args.rows
    device = torch.device(args.device)
    indptr, indices, values = make_csr(rows, F, args.density, args.seed)
    nnz = int(indptr[-1])
    res = {"features": F, "density": args.density, "rows": rows, "nnz": nnz, "trees": args.trees, "depth": args.depth,
           "micro_batch": args.micro_batch, "reps": args.reps, "device": torch.cuda.get_device_name(device),
           "dense_bytes_per_row": 4 * F, "csr_bytes_per_row": round(8 * nnz / rows + 4, 1)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "gbdt.pmml")
        with open(path, "w") as fh:
            fh.write(gbdt_pmml(n_trees=args.trees, depth=args.depth, n_features=F, seed=args.seed + 1))
        dense_scores = sparse_scores = None
        if args.mode in ("both", "dense"):
            X = dense_pinned(indptr, indices, values, rows, F)
            rate, pb = end_to_end(RecordBatch(X), path, device, args.warmup, args.reps, args.micro_batch)
            res["dense_rows_per_s"] = round(rate)
            res["dense_h2d_gbps"] = round(rate * 4 * F / 1e9, 2)
            dense_scores = (pb.scores.copy(), pb.valid.copy())
            del X, pb
        if args.mode in ("both", "sparse"):
            from flink_jpmml_amd.api.batch import SparseRecordBatch

            sb = SparseRecordBatch(pinned_like(indptr.astype(np.int32)), pinned_like(indices), pinned_like(values), F,
                                   validated=True)
            rate, pb = end_to_end(sb, path, device, args.warmup, args.reps, args.micro_batch)
            res["sparse_rows_per_s"] = round(rate)
            res["sparse_h2d_gbps"] = round(rate * (8 * nnz / rows + 4) / 1e9, 2)
            sparse_scores = (pb.scores.copy(), pb.valid.copy())
            del pb
        if dense_scores is not None and sparse_scores is not None:
            res["sparse_over_dense"] = round(res["sparse_rows_per_s"] / res["dense_rows_per_s"], 3)
            res["scores_bit_equal"] = bool(np.array_equal(dense_scores[1], sparse_scores[1]) and np.array_equal(
                dense_scores[0].view(np.uint32), sparse_scores[0].view(np.uint32)))
        if args.mode != "dense" and not args.no_kernels:
            from flink_jpmml_amd.ops.sparse import csr_expand
            from flink_jpmml_amd.runtime.compiled import CompiledPmml

            m = min(rows, args.micro_batch)
            k = int(indptr[m])
            ip = torch.from_numpy(indptr[:m + 1].astype(np.int32)).to(device)
            ix = torch.from_numpy(indices[:k]).to(device)
            va = torch.from_numpy(values[:k]).to(device)
            out = torch.empty((m, F), dtype=torch.float32, device=device)
            with open(path) as fh:
                plan = CompiledPmml.from_string(fh.read()).plan(device)
            s, v = plan.alloc_outputs(m)
            sync = torch.cuda.synchronize
            res["kernel_rows"] = m
            res["fill_ms"] = round(event_ms(lambda: out.fill_(float("nan")), sync, 20), 4)
            res["expand_ms"] = round(event_ms(lambda: csr_expand(ip, ix, va, out, k), sync, 20), 4)
            res["model_ms"] = round(event_ms(lambda: plan.launch(out, s, v), sync, 20), 4)
            res["expand_over_fill"] = round(res["expand_ms"] / res["fill_ms"], 2)
            res["expand_write_gbps"] = round(m * F * 4 / res["expand_ms"] / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
