"""Forests and chains of more than 16 classes on the device: ``tree_classes_kernel``
(ops/csrc/tree_classes.hip) against the route each model took before the kernel.

* a 26-class majority-vote forest, 500 trees of depth 8 over 32 fields: ``TreePlan`` refused it and
  so did every segment of the segmented fallback, so it scored on the float64 host oracle;
* a 20-class boosted chain (20 ensembles of 25 trees, depth 6, softmax): ``ChainPlan``, one launch
  per class ensemble plus tensor operations.

1M standard-normal fp32 rows resident in HBM. Timed with device events over ``REPEAT`` launches
after ``WARMUP``; the median is reported. The host oracle is timed on a slice and reported per
million rows. Run from the repository root on a machine with a GPU::

    python profiles/class_forest/measure.py [rows] > results.json
"""

import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = 2_000
WARMUP, REPEAT = 3, 10


def timed(fn):
    import torch

    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEAT):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main() -> None:
    import torch

    from flink_jpmml_amd.bench import synth
    from flink_jpmml_amd.runtime.compiled import CompiledPmml
    from flink_jpmml_amd.runtime.segmented import ChainPlan

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "warmup": WARMUP, "repeat": REPEAT,
           "host_rows_timed": HOST_ROWS, "cases": {}}
    cases = [("vote_forest_26x500x8", synth.random_forest_pmml(n_trees=500, depth=8, n_features=32, n_classes=26)),
             ("chain_20x25x6", synth.gbdt_pmml(n_trees=25, depth=6, n_features=32, objective="multiclass",
                                               n_classes=20))]
    X = torch.randn((ROWS, 32), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(1))
    for name, text in cases:
        c = CompiledPmml.from_string(text)
        plan = c.plan(dev)
        assert plan.kind == "tree_classes", plan.kind
        s, v = plan.alloc_outputs(ROWS)
        probs = torch.empty((ROWS, plan.C), dtype=torch.float32, device=dev)
        entry = {"classes": plan.C, "trees": plan.n_trees, "depth": plan.depth, "staged_columns": plan.n_stage,
                 "leaf_form": "dense" if plan.dense else "pair",
                 "tree_classes_kernel": timed(lambda: plan.launch(X, s, v)),
                 "tree_classes_kernel_with_probs": timed(lambda: plan.launch(X, s, v, probs=probs))}
        if name.startswith("chain"):
            before = ChainPlan(c, dev)
            s2, v2 = before.alloc_outputs(ROWS)
            entry["chain_plan"] = timed(lambda: before.launch(X, s2, v2))
            torch.cuda.synchronize()
            entry["chain_plan_rows_with_another_label"] = int((s2 != s).sum().item())
        Xh = X[:HOST_ROWS].cpu().numpy()
        t0 = time.perf_counter()
        so, vo = c.score_matrix_oracle(Xh)
        entry["host_oracle_seconds_per_million_rows"] = (time.perf_counter() - t0) * 1e6 / HOST_ROWS
        sd, vd = s[:HOST_ROWS].cpu().numpy(), v[:HOST_ROWS].cpu().numpy().astype(bool)
        entry["host_compared"] = {"rows_with_another_validity": int((np.asarray(vo, bool) != vd).sum()),
                                  "rows_with_another_label": int((sd[vd] != np.asarray(so, np.float32)[vd]).sum())}
        res["cases"][name] = entry
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, ".")
    main()
