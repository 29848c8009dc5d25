"""Output-field kernel against a torch-op composition, and ``predict_records`` with and without
``outputs=True``, at 1M rows on one GPU (device events, warmed up).

Two models: the 500-tree depth-8 3-class forest with ``predictedValue`` + 3 probabilities, and a
16-class forest with ``top_k=3``. Prints one JSON line per model; the figures recorded in
``profiles/outputs/README.md`` come from this script.

    python scripts/outputs_bench.py [--rows 1000000] [--iters 2000] [--warmup 10]
"""

import argparse
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def with_output(text: str, fields: str) -> str:
    end = text.index("</MiningSchema>") + len("</MiningSchema>")
    rest = re.sub(r"\A\s*<Output>.*?</Output>", "", text[end:], count=1, flags=re.S)
    return text[:end] + f"\n<Output>{fields}</Output>\n" + rest


def output_fields(n_classes: int) -> str:
    label = '<OutputField name="label" optype="categorical" dataType="integer" feature="predictedValue"/>'
    probs = "".join(f'<OutputField name="p_{c}" optype="continuous" dataType="double" feature="probability" '
                    f'value="{c}"/>' for c in range(n_classes))
    return label + probs


def timed(fn, iters: int, warmup: int) -> float:
    """Mean milliseconds of ``fn()`` between two device events, after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_composition(plan, raw_s, raw_v, probs):
    """The same columns from torch ops: gather through the encoding tables, ``where`` on validity,
    a stable descending ``sort`` for the ranks (the baseline the kernel is measured against)."""
    nan = torch.full((), float("nan"), device=raw_s.device)
    ok = raw_v != 0
    okidx = ok & ~torch.isnan(raw_s)
    cols = []
    for op, arg, off, _ in plan.prog_np.tolist():
        if op == 1:  # TABLE
            idx = torch.where(okidx & (raw_s >= 0) & (raw_s < arg), raw_s, torch.full_like(raw_s, float(arg))).long()
            cols.append(plan.tables[off: off + arg + 1][idx])
        elif op == 2:  # PROB
            cols.append(torch.where(ok, probs[:, arg], nan))
        elif op in (7, 8):
            continue  # the top-k block below
        else:
            raise SystemExit(f"outputs_bench: op {op} is not part of these models")
    out = [torch.stack(cols, dim=1)]
    if plan.top_k:
        # NaN never ranks; ties to the lower class is what a stable descending sort gives
        p = torch.where(torch.isnan(probs), torch.full_like(probs, float("-inf")), probs)
        tp, ti = torch.sort(p, dim=1, descending=True, stable=True)
        tp, ti = tp[:, : plan.top_k], ti[:, : plan.top_k]
        keep = ok[:, None] & (tp > float("-inf"))
        out.append(torch.where(keep, ti.float(), nan))
        out.append(torch.where(keep, tp, nan))
    lt = plan.label_table
    L = lt.numel() - 1
    idx = torch.where(okidx & (raw_s >= 0) & (raw_s < L), raw_s, torch.full_like(raw_s, float(L))).long()
    s = lt[idx]
    v = ok & ~torch.isnan(s)
    return torch.cat(out, dim=1), torch.where(v, s, nan), v


def run(name: str, text: str, top_k: int, args) -> dict:
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.bench.synth import stream_matrix
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.ops.outputs import outputs_launch

    dev = torch.device("cuda:0")
    model = PmmlModel.from_string(text).bind(dev, ScoringConfig(device=dev, fallback="error"))
    compiled = model.compiled
    plan = compiled.output_plan(dev, top_k=top_k)
    n = args.rows
    X = stream_matrix(n, compiled.n_features, seed=5, missing_rate=0.02)
    Xd = torch.from_numpy(X).to(dev)
    raw_s = torch.empty(n, dtype=torch.float32, device=dev)
    raw_v = torch.empty(n, dtype=torch.uint8, device=dev)
    probs = torch.empty((n, plan.C), dtype=torch.float32, device=dev)
    plan.inner.launch(Xd, raw_s, raw_v, probs=probs)
    moved = 4 * n * ((plan.C or 0) + plan.n_col) + 10 * n  # probs in, columns out, score / valid in and out
    # enough copies of every buffer that a pass over all of them is larger than the 256 MiB last-level
    # cache: the rotating figures read and write HBM, the "hot" ones one cache-resident set
    sets = -(-(768 << 20) // moved)
    ins = [(raw_s, raw_v, probs)] + [(raw_s.clone(), raw_v.clone(), probs.clone()) for _ in range(sets - 1)]
    outs = [(torch.empty((n, plan.n_col), dtype=torch.float32, device=dev),
             torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))
            for _ in range(sets)]
    turn = [0]

    def kernel(rotate=True):
        i = turn[0] = (turn[0] + 1) % sets if rotate else 0
        (s_, v_, p_), (o_, so_, vo_) = ins[i], outs[i]
        outputs_launch(s_, v_, o_, plan.prog, plan.tables, probs=p_, label_table=plan.label_table,
                       k=top_k, score_out=so_, valid_out=vo_)

    def composed(rotate=True):
        i = turn[0] = (turn[0] + 1) % sets if rotate else 0
        return torch_composition(plan, *ins[i])

    def issue_only():
        # the same call over 256 rows: what back-to-back launches cost to issue from Python (argument
        # checks, struct fill, the launch itself); a 1M-row figure near it measures the host
        (s_, v_, p_), (o_, so_, vo_) = ins[0], outs[0]
        outputs_launch(s_[:256], v_[:256], o_[:256], plan.prog, plan.tables, probs=p_[:256],
                       label_table=plan.label_table, k=top_k, score_out=so_[:256], valid_out=vo_[:256])

    kernel_ms = timed(kernel, args.iters, args.warmup)
    kernel_hot_ms = timed(lambda: kernel(False), args.iters, args.warmup)
    issue_ms = timed(issue_only, args.iters, args.warmup)
    torch_ms = timed(composed, max(20, args.iters // 10), args.warmup)
    torch_hot_ms = timed(lambda: composed(False), max(20, args.iters // 10), args.warmup)
    ref, rs, rv = composed(False)
    kernel(False)
    torch.cuda.synchronize()
    out, so, vo = outs[0]
    same = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32))
                and torch.equal(so.view(torch.int32), rs.view(torch.int32)) and torch.equal(vo.bool(), rv))
    del ins, outs

    Xp = torch.from_numpy(X).pin_memory()
    rates = {}
    for label, kw in (("plain", {}), ("outputs", dict(outputs=True, top_k=top_k))):
        for _ in range(3):
            model.predict_records(RecordBatch(Xp), **kw).wait()
        t0 = time.perf_counter()
        for _ in range(args.stream_iters):
            model.predict_records(RecordBatch(Xp), **kw).wait()
        rates[label] = n * args.stream_iters / (time.perf_counter() - t0)
    return dict(model=name, rows=n, classes=plan.C, columns=plan.n_col, top_k=top_k,
                buffer_sets=sets, bytes_per_call=moved,
                kernel_ms=round(kernel_ms, 4), torch_ms=round(torch_ms, 4), torch_over_kernel=round(torch_ms / kernel_ms, 2),
                kernel_gb_s=round(moved / kernel_ms / 1e6, 1), kernel_hot_ms=round(kernel_hot_ms, 4),
                torch_hot_ms=round(torch_hot_ms, 4), issue_floor_ms=round(issue_ms, 4), bit_equal_to_torch=same,
                predict_records_rows_s=round(rates["plain"]), predict_records_outputs_rows_s=round(rates["outputs"]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=2000, help="timed kernel launches (a tenth as many compositions)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stream-iters", type=int, default=100, help="timed predict_records calls")
    args = ap.parse_args()
    from flink_jpmml_amd.bench.synth import random_forest_pmml

    cases = [
        ("forest 500x8, 3 classes, label + 3 probabilities",
         with_output(random_forest_pmml(500, 8, 32, 3, seed=0), output_fields(3)), 0),
        ("forest 100x8, 16 classes, label + 16 probabilities, top_k=3",
         with_output(random_forest_pmml(100, 8, 32, 16, seed=0), output_fields(16)), 3),
    ]
    for name, text, top_k in cases:
        print(json.dumps(run(name, text, top_k, args)), flush=True)


if __name__ == "__main__":
    main()
