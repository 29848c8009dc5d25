"""Reason-code ranking on the device: kernel time, whole ``OutputPlan.launch`` and the two baselines.

Workload: a 32-characteristic, 4-attribute scorecard (three ``lessThan`` bins and a ``True``
attribute per field), 1M standard-normal fp32 rows resident in HBM. Two documents: every
characteristic with its own code (the register path) and 8 codes shared by 4 characteristics each
(the accumulator path); ranks 1 (K = 1) and 1 … 3 (K = 4 instantiation).

Timed with device events over ``REPEAT`` launches after ``WARMUP``; the median is reported. Run from
the repository root on a machine with a GPU::

    python profiles/reasons/measure.py [rows] > results.json
"""

import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = 100_000  # the host path ranks row by row in Python: timed on a slice, reported per row
WARMUP, REPEAT = 3, 20
N_CHAR, N_ATTR = 32, 4


def document(shared: bool, ranks, use_reason_codes: bool = True) -> str:
    from flink_jpmml_amd.bench.synth import reason_scorecard_pmml

    rng = np.random.default_rng(7)
    chars = []
    for j in range(N_CHAR):
        cuts = np.sort(rng.normal(size=N_ATTR - 1))
        attrs = [{"predicate": f'<SimplePredicate field="f{j}" operator="lessThan" value="{float(np.float32(c))!r}"/>',
                  "partial": float(np.round(rng.uniform(0, 20), 2))} for c in cuts]
        attrs.append({"predicate": "<True/>", "partial": float(np.round(rng.uniform(0, 20), 2))})
        chars.append({"name": f"ch{j}", "reason_code": f"R{j % 8 if shared else j}", "baseline": None,
                      "attributes": attrs})
    return reason_scorecard_pmml(chars, n_features=N_CHAR, ranks=ranks, baseline=10.0,
                                 use_reason_codes=use_reason_codes)


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
    from flink_jpmml_amd.ops.reasons import geometry, reasons_launch, template_k

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    Xh = rng.standard_normal((ROWS, N_CHAR), dtype=np.float32)
    X = torch.from_numpy(Xh).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "characteristics": N_CHAR, "attributes": N_ATTR,
           "warmup": WARMUP, "repeat": REPEAT, "cases": {}}

    def run_plan(plan):
        score, valid = plan.alloc_outputs(ROWS)
        matrix = plan.alloc_matrix(ROWS)
        t = timed(lambda: plan.launch(X, score, valid, outputs=matrix))
        return t, score, valid, matrix

    # (a) the score alone: the same scorecard without reason codes, through the default call
    plain = PmmlModel.from_string(document(False, ())).compiled
    res["score_alone_output_plan"], _, _, _ = run_plan(plain.output_plan(dev))
    off = PmmlModel.from_string(document(False, (1, 2, 3), use_reason_codes=False)).compiled
    res["use_reason_codes_false_output_plan"], _, _, _ = run_plan(off.output_plan(dev, reason_codes=True))
    tree = plain.plan(dev)
    s0, v0 = tree.alloc_outputs(ROWS)
    res["general_tree_kernel"] = timed(lambda: tree.launch(X, s0, v0))
    res["general_tree_plan"] = type(tree).__name__ + ":" + str(getattr(tree, "layout", ""))

    for shared in (False, True):
        for ranks in ((1,), (1, 2, 3)):
            compiled = PmmlModel.from_string(document(shared, ranks)).compiled
            plan = compiled.output_plan(dev, reason_codes=True)
            whole, score, valid, matrix = run_plan(plan)
            T = plan.reasons
            kern = timed(lambda: reasons_launch(X, valid, matrix, T, prep=plan._reason_prep))
            rows, feat_lds = geometry(T.n_feat, T.n_code, T.shared)
            key = f"{'shared' if shared else 'disjoint'}_k{len(ranks)}"
            entry = {"reason_kernel": kern, "output_plan_launch": whole, "template_k": template_k(T.k),
                     "codes": T.n_code, "rows_per_workgroup": rows, "features_in_lds": feat_lds}
            # the same rows on the host: what a user gets without the switch
            t0 = time.perf_counter()
            _, hv, host = PmmlModel.from_string(document(shared, ranks)).predict_batch_outputs(Xh[:HOST_ROWS])
            entry["host_seconds_per_million_rows"] = (time.perf_counter() - t0) * 1e6 / HOST_ROWS
            entry["host_rows_timed"] = HOST_ROWS
            got = matrix[:HOST_ROWS].cpu().numpy().astype(np.float64)
            want = np.asarray(host.matrix)
            dec = [[compiled.schema.decode(n, float(v)) for v in got[:, j]] for j, n in enumerate(plan.names)]
            entry["equal_to_host_on_timed_rows"] = bool(
                np.array_equal(valid[:HOST_ROWS].cpu().numpy() != 0, hv)
                and all(dec[j] == host.decode(n) for j, n in enumerate(plan.names)) and got.shape == want.shape)
            res["cases"][key] = entry
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, ".")
    main()
