"""Class outputs of a k-NN classifier on the device: the class-output instantiation of ``knn.hip``
against the scoring instantiation, the whole ``OutputPlan.launch`` and the host path.

A 5-NN classifier over 1024 instances x 16 fields (euclidean, so ``auto`` takes the MFMA kernel),
``weightedMajorityVote``, with 3 and with 256 classes, over 1M standard-normal fp32 rows resident in
HBM. The document asks ``predictedValue``, the winner's ``probability``, the ``probability`` of two
named classes and ``top_k = 3``.

For each class count and kernel variant: the scoring plan's launch (``knn_kernel`` /
``knn_mfma_kernel`` as before this switch: one score per row), the index-mode plan's launch (label
index + the ``[rows, C]`` vote shares), the whole ``OutputPlan.launch``, and the host path on a slice.

Timed with device events over ``REPEAT`` launches after ``WARMUP``; the median is reported. Run from
the repository root on a machine with a GPU::

    python profiles/knn_classes/measure.py [rows] > results.json
"""

import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = 20_000  # the host path builds [n, N] float64 matrices: timed on a slice, reported per million
WARMUP, REPEAT = 3, 10
TOP_K = 3


def document(classes: int) -> str:
    from flink_jpmml_amd.bench import synth

    text = synth.knn_pmml(1024, 16, k=5, seed=1, metric="euclidean", classes=classes,
                          method="weightedMajorityVote")
    prob = '<OutputField name="{}" feature="probability"{} optype="continuous" dataType="double"/>'
    fields = ['<OutputField name="label" feature="predictedValue" optype="categorical" dataType="string"/>',
              prob.format("p_win", ""), prob.format("p_0", ' value="0"'), prob.format("p_1", ' value="1"')]
    return text.replace("</MiningSchema>", "</MiningSchema>\n  <Output>" + "".join(fields) + "</Output>", 1)


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

    from flink_jpmml_amd.api.pmml_model import PmmlModel

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "warmup": WARMUP, "repeat": REPEAT, "cases": {}}
    Xh = np.random.default_rng(1).standard_normal((ROWS, 16), dtype=np.float32)
    X = torch.from_numpy(Xh).to(dev)
    for classes in (3, 256):
        text = document(classes)
        model = PmmlModel.from_string(text)
        compiled = model.compiled
        entry = {}
        for variant in ("mfma", "valu"):
            base = compiled.plan(dev, knn_variant=variant)
            s0, v0 = base.alloc_outputs(ROWS)
            plan = compiled.output_plan(dev, knn_classes=True, top_k=TOP_K, knn_variant=variant)
            inner = plan.inner
            s1, v1 = inner.alloc_outputs(ROWS)
            probs = torch.empty((ROWS, plan.C), dtype=torch.float32, device=dev)
            score, valid = plan.alloc_outputs(ROWS)
            matrix = plan.alloc_matrix(ROWS)
            entry[variant] = {
                "variant": inner.variant, "k": inner.k, "classes": plan.C,
                "scoring_kernel": timed(lambda: base.launch(X, s0, v0)),
                "class_output_kernel": timed(lambda: inner.launch(X, s1, v1, probs=probs)),
                "output_plan_launch": timed(lambda: plan.launch(X, score, valid, outputs=matrix)),
                "probs_megabytes": ROWS * plan.C * 4 / 1e6,
            }
            if variant == "mfma":
                got = matrix.cpu().numpy()
            del probs, matrix
            torch.cuda.empty_cache()
        # the host path: what a user gets without the switch
        t0 = time.perf_counter()
        _, _, host = model.predict_batch_outputs(Xh[:HOST_ROWS], top_k=TOP_K)
        entry["host_seconds_per_million_rows"] = (time.perf_counter() - t0) * 1e6 / HOST_ROWS
        entry["host_rows_timed"] = HOST_ROWS
        want = np.asarray(host.matrix)
        n_out = want.shape[1]
        entry["host_compared"] = {
            "rows_with_another_label": int((got[:HOST_ROWS, 0] != want[:, 0]).sum()),
            "max_abs_probability_difference": float(np.abs(got[:HOST_ROWS, 1:n_out] - want[:, 1:]).max()),
            "rows_with_another_top_k": int((got[:HOST_ROWS, n_out: n_out + TOP_K] != host.top_index).any(axis=1).sum())}
        res["cases"][f"classes_{classes}"] = entry
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, ".")
    main()
