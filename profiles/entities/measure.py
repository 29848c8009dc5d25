"""Ranked entities on the device: kernel time, whole ``OutputPlan.launch`` and the baselines.

Three documents over 1M standard-normal fp32 rows resident in HBM:

* ``kmeans_named64``: 64 centres x 32 fields, the affinity of all 64 clusters named;
* ``kmeans_ranks3``: the same model, ``clusterId`` and affinity of ranks 1 ... 3;
* ``knn5``: a 5-NN regression over 1024 instances x 16 fields, 5 neighbour ids and distances.

For each: the entity kernel alone, the whole ``OutputPlan.launch``, the same plan without entity
fields (``predictedValue`` and, for the k-means, the winner's affinity: what lowered before), the same
columns from device tensor ops (distance matrix + ``torch.topk`` + gathers) with their outputs
compared, and the host path on a slice.

Timed with device events over ``REPEAT`` launches after ``WARMUP``; the median is reported. Run from
the repository root on a machine with a GPU::

    python profiles/entities/measure.py [rows] > results.json
"""

import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = 20_000  # the host path builds [n, N] float64 matrices: timed on a slice, reported per million
WARMUP, REPEAT = 3, 10


def _output(fields) -> str:
    return "</MiningSchema>\n  <Output>" + "".join(fields) + "</Output>"


def _field(name, feature, rank=1, value=None, dtype="double") -> str:
    optype = "continuous" if dtype == "double" else "categorical"
    val = f' value="{value}"' if value is not None else ""
    return f'<OutputField name="{name}" feature="{feature}" rank="{rank}"{val} optype="{optype}" dataType="{dtype}"/>'


def documents():
    from flink_jpmml_amd.bench import synth

    km = synth.kmeans_pmml(64, 32, seed=1)
    knn = synth.knn_pmml(1024, 16, k=5, classification=False, seed=1, metric="euclidean")
    label = _field("label", "predictedValue", dtype="string")
    win = _field("aff", "affinity")
    ranked = lambda feat, ks: [f for r in ks for f in (_field(f"id{r}", feat, r, dtype="integer"),
                                                       _field(f"aff{r}", "affinity", r))]
    return {
        "kmeans_named64": (km.replace("</MiningSchema>", _output(
            [label] + [_field(f"a{k + 1}", "affinity", value=str(k + 1)) for k in range(64)]), 1),
            km.replace("</MiningSchema>", _output([label, win]), 1), 32),
        "kmeans_ranks3": (km.replace("</MiningSchema>", _output([label] + ranked("clusterId", (1, 2, 3))), 1),
                          km.replace("</MiningSchema>", _output([label, win]), 1), 32),
        "knn5": (knn.replace("</MiningSchema>", _output([_field("y", "predictedValue")]
                                                        + ranked("entityId", range(1, 6))), 1),
                 knn.replace("</MiningSchema>", _output([_field("y", "predictedValue")]), 1), 16),
    }


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


def tensor_ops(T, X, k: int, chunk: int = 1 << 17):
    """The same columns from device tensor ops, complete rows only (no missing-value rescale):
    ``[chunk, N]`` distances by the expansion, ``torch.topk`` (smallest), gathers."""
    import torch

    E = torch.from_numpy(T.ent).to(X.device)
    w = torch.from_numpy(T.weights).to(X.device)
    wc, cc = (E * w).t().contiguous(), (E * E * w).sum(dim=1)
    ids, affs, full = [], [], []
    for r0 in range(0, X.shape[0], chunk):
        x = X[r0: r0 + chunk]
        d = ((x * x * w).sum(dim=1, keepdim=True) - 2.0 * (x @ wc) + cc).clamp_min_(0.0)
        if T.metric == 1:
            d = d.sqrt_()
        top = torch.topk(d, k, dim=1, largest=False, sorted=True)
        ids.append(top.indices)
        affs.append(top.values)
        full.append(d)
    return torch.cat(ids), torch.cat(affs), full


def main() -> None:
    import torch

    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.ops.entities import entities_launch, template_k

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "warmup": WARMUP, "repeat": REPEAT, "cases": {}}
    for name, (text, before, F) in documents().items():
        Xh = np.random.default_rng(1).standard_normal((ROWS, F), dtype=np.float32)
        X = torch.from_numpy(Xh).to(dev)

        def run_plan(plan):
            score, valid = plan.alloc_outputs(ROWS)
            matrix = plan.alloc_matrix(ROWS)
            return timed(lambda: plan.launch(X, score, valid, outputs=matrix)), matrix

        compiled = PmmlModel.from_string(text).compiled
        plan = compiled.output_plan(dev, entity_ranks=True)
        whole, matrix = run_plan(plan)
        T = plan.entities
        entry = {"plan": type(plan.inner).__name__, "variant": T.variant, "template_k": template_k(T.k), "k": T.k,
                 "columns": len(T.cols), "rows_per_workgroup": T.rows, "output_plan_launch": whole,
                 "entity_kernel": timed(lambda: entities_launch(X, matrix, T, prep=plan.inner.prep))}
        entry["output_plan_without_entity_fields"], _ = run_plan(PmmlModel.from_string(before).compiled.output_plan(dev))
        base = compiled.plan(dev)
        s0, v0 = base.alloc_outputs(ROWS)
        entry["model_kernel"] = timed(lambda: base.launch(X, s0, v0))
        # device tensor ops
        k = T.k
        entry["tensor_ops"] = timed(lambda: tensor_ops(T, X, k))
        ids, affs, full = tensor_ops(T, X, k)
        got = matrix.cpu().numpy()
        col = {n: got[:, i] for i, n in enumerate(plan.names)}
        cmp = {}
        if name == "kmeans_named64":
            d = torch.cat(full).cpu().numpy()
            mine = np.stack([col[f"a{j + 1}"] for j in range(64)], axis=1)
            cmp["max_abs_difference"] = float(np.abs(mine - d).max())
        else:
            n_rank = 3 if name == "kmeans_ranks3" else 5
            mine_id = np.stack([col[f"id{r}"] for r in range(1, n_rank + 1)], axis=1) - 1
            mine_aff = np.stack([col[f"aff{r}"] for r in range(1, n_rank + 1)], axis=1)
            cmp["rows_with_another_entity"] = int((mine_id != ids.cpu().numpy()[:, :n_rank]).any(axis=1).sum())
            cmp["max_abs_affinity_difference"] = float(np.abs(mine_aff - affs.cpu().numpy()[:, :n_rank]).max())
        entry["tensor_ops_compared"] = cmp
        del full, ids, affs
        # the host path: what a user gets without the switch
        t0 = time.perf_counter()
        _, _, host = PmmlModel.from_string(text).predict_batch_outputs(Xh[:HOST_ROWS])
        entry["host_seconds_per_million_rows"] = (time.perf_counter() - t0) * 1e6 / HOST_ROWS
        entry["host_rows_timed"] = HOST_ROWS
        want = np.asarray(host.matrix)
        aff_cols = [i for i, n in enumerate(plan.names) if n.startswith("a")]
        id_cols = [i for i, n in enumerate(plan.names) if n.startswith("id")]
        entry["host_compared"] = {
            "max_abs_affinity_difference": float(np.abs(got[:HOST_ROWS][:, aff_cols] - want[:, aff_cols]).max()),
            "rows_with_another_entity": int((got[:HOST_ROWS][:, id_cols] != want[:, id_cols]).any(axis=1).sum())
            if id_cols else 0}
        res["cases"][name] = entry
        del X, matrix
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, ".")
    main()
