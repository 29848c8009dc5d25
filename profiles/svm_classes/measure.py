"""Class outputs of an SVM classifier on the device: the class-output instantiations of ``svm.hip``
against the scoring instantiations, the whole ``OutputPlan.launch`` and the host path.

Four synthetic classifiers (``bench/synth.py::svm_pmml``, RBF kernel) over 1M standard-normal fp32 rows
resident in HBM:

* ``rbf256``: binary, 256 support vectors, 16 fields (``svm_mfma_kernel``, one machine);
* ``ovo12``: 12 classes one-against-one, 66 machines, 1024 support vectors, 64 fields (``svm_wide_kernel``);
* ``ovo100``: 100 classes one-against-one, 4950 machines, 512 support vectors, 16 fields (``svm_wide_kernel``);
* ``gemm5``: 5 classes one-against-one, 256 support vectors, 16 fields on ``SvmGemmPlan`` (tensor ops).

Each document asks ``predictedValue``, the winner's ``probability``, the ``probability`` of two named
classes and ``top_k = 3``. Per model: the scoring plan's launch (one score per row, the code before
this switch), the index-mode plan's launch (class index + the ``[rows, C]`` vote shares) and the whole
``OutputPlan.launch``, alternated launch by launch in the same run, and the host path on a slice.

Timed with device events over ``REPEAT`` rounds after ``WARMUP``; the median is reported. Run from the
repository root on a machine with a GPU::

    python profiles/svm_classes/measure.py [rows] > results.json
"""

import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = 20_000  # the host path builds [n, support vectors] float64 matrices: timed on a slice
WARMUP, REPEAT = 3, 10
TOP_K = 3

MODELS = {
    "rbf256": (dict(n_features=16, n_sv=256, seed=1, n_classes=2), {}),
    "ovo12": (dict(n_features=64, n_sv=1024, seed=1, n_classes=12), {}),
    "ovo100": (dict(n_features=16, n_sv=512, seed=1, n_classes=100), {}),
    "gemm5": (dict(n_features=16, n_sv=256, seed=1, n_classes=5), {"svm_impl": "gemm"}),
}


def document(**kw) -> str:
    from flink_jpmml_amd.bench import synth

    text = synth.svm_pmml(kernel="radialBasis", gamma=0.05, **kw)
    prob = '<OutputField name="{}" feature="probability"{} optype="continuous" dataType="double"/>'
    fields = ['<OutputField name="label" feature="predictedValue" optype="categorical" dataType="string"/>',
              prob.format("p_win", ""), prob.format("p_0", ' value="0"'), prob.format("p_1", ' value="1"')]
    return text.replace("</MiningSchema>", "</MiningSchema>\n  <Output>" + "".join(fields) + "</Output>", 1)


def timed_alternating(fns: dict) -> dict:
    """Every function once per round, round after round: neighbours in time share the device's state."""
    import torch

    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPEAT):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
            for k, v in ms.items()}


def base_of(plan):
    while getattr(plan, "inner", None) is not None:
        plan = plan.inner
    return plan


def main() -> None:
    import torch

    from flink_jpmml_amd.api.pmml_model import PmmlModel

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "warmup": WARMUP, "repeat": REPEAT, "cases": {}}
    for name, (kw, opts) in MODELS.items():
        F = kw["n_features"]
        Xh = np.random.default_rng(1).standard_normal((ROWS, F), dtype=np.float32)
        X = torch.from_numpy(Xh).to(dev)
        model = PmmlModel.from_string(document(**kw))
        compiled = model.compiled
        base = compiled.plan(dev, **opts)
        s0, v0 = base.alloc_outputs(ROWS)
        plan = compiled.output_plan(dev, svm_classes=True, top_k=TOP_K, **opts)
        inner = plan.inner
        s1, v1 = inner.alloc_outputs(ROWS)
        probs = torch.empty((ROWS, plan.C), dtype=torch.float32, device=dev)
        score, valid = plan.alloc_outputs(ROWS)
        matrix = plan.alloc_matrix(ROWS)
        kernel = base_of(inner)
        entry = {"plan": type(kernel).__name__, "classes": plan.C,
                 "machines": len(compiled.evaluator.sm.machines), "support_vectors": kw["n_sv"], "fields": F,
                 "probs_megabytes": ROWS * plan.C * 4 / 1e6}
        entry.update(timed_alternating({
            "scoring_kernel": lambda: base.launch(X, s0, v0),
            "class_output_kernel": lambda: inner.launch(X, s1, v1, probs=probs),
            "output_plan_launch": lambda: plan.launch(X, score, valid, outputs=matrix)}))
        got = matrix[:HOST_ROWS].cpu().numpy()
        del probs, matrix, X
        torch.cuda.empty_cache()
        # the host path: what a user gets without the switch
        t0 = time.perf_counter()
        _, _, host = model.predict_batch_outputs(Xh[:HOST_ROWS], top_k=TOP_K)
        entry["host_seconds_per_million_rows"] = (time.perf_counter() - t0) * 1e6 / HOST_ROWS
        entry["host_rows_timed"] = HOST_ROWS
        want = np.asarray(host.matrix)
        n_out = want.shape[1]
        same = (got[:, 0] == want[:, 0])  # rows on which every machine voted as on the host have equal shares
        entry["host_compared"] = {
            "rows_with_another_label": int((~same).sum()),
            "max_abs_probability_difference": float(np.nanmax(np.abs(got[:, 1:n_out] - want[:, 1:]))),
            "rows_with_another_top_k": int((np.nan_to_num(got[:, n_out: n_out + TOP_K], nan=-1.0)
                                            != host.top_index).any(axis=1).sum())}
        res["cases"][name] = entry
        print(name, json.dumps(entry), file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, ".")
    main()
