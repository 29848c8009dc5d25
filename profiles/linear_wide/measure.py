"""Wide regression tables on the device: ``linear_wide_kernel`` (ops/csrc/linear_wide.hip) against
torch's own GEMM with a torch epilogue, and against the float64 host oracle (the path these models
took before the kernel: ``LinearPlan`` refuses more than 16 tables x 128 fields).

Shapes (tables x fields): 20 x 123 — the design matrix of ``synth.naive_bayes_pmml(n_features=40,
classes=20)``, timed on its inner plan over a resident design matrix; 40 x 200 softmax; 256 x 256
softmax with and without the ``[rows, 256]`` probabilities; 1 x 1024 regression. 1M standard-normal
fp32 rows resident in HBM, standard-normal coefficients.

Timed with device events over ``REPEAT`` launches after ``WARMUP``; the median is reported. FLOP/s and
bytes/s follow from the shapes (2 rows F K; rows (4 F + 5 + 4 C with probabilities)); ``bound`` names
the larger of the two roofline times at 157.3 TFLOP/s fp32 matrix and 8 TB/s HBM (data sheet).
Run from the repository root on a machine with a GPU::

    python profiles/linear_wide/measure.py [rows] > results.json
"""

import io
import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = 2_000  # the host oracle is timed on a slice and reported per million rows
WARMUP, REPEAT = 3, 10
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12


def document(F: int, K: int, norm: str, seed: int = 1) -> str:
    """A dense ``RegressionModel``: ``K`` tables (0: one regression table) over ``F`` numeric fields."""
    from flink_jpmml_amd.bench.synth import _data_dictionary, _header, _mining_schema

    rng = np.random.default_rng(seed)
    T = max(K, 1)
    W = rng.standard_normal((F, T)).astype(np.float32) / np.float32(np.sqrt(F))
    out = io.StringIO()
    _header(out, f"wide regression {F} x {K} {norm}")
    cats = [str(k) for k in range(K)] if K else None
    _data_dictionary(out, F, "y", "integer" if K else "double", cats)
    fn = "classification" if K else "regression"
    out.write(f' <RegressionModel functionName="{fn}" normalizationMethod="{norm}">\n')
    _mining_schema(out, F, "y", "  ")
    for k in range(T):
        tc = f' targetCategory="{cats[k]}"' if cats else ""
        out.write(f'  <RegressionTable intercept="{float(k % 5 - 2)!r}"{tc}>')
        out.write("".join(f'<NumericPredictor name="f{f}" coefficient="{float(W[f, k])!r}"/>' for f in range(F)))
        out.write('</RegressionTable>\n')
    out.write(' </RegressionModel>\n</PMML>\n')
    return out.getvalue()


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


def roofline(ms: float, F: int, K: int, C: int) -> dict:
    flops, nbytes = 2.0 * ROWS * F * K, ROWS * (4.0 * F + 5 + 4 * C)
    t = ms * 1e-3
    return {"tflops": flops / t / 1e12, "terabytes_per_s": nbytes / t / 1e12,
            "bound": "memory" if nbytes / PEAK_BYTES >= flops / PEAK_FLOPS else "compute",
            "fraction_of_that_roof": max(nbytes / PEAK_BYTES, flops / PEAK_FLOPS) / t}


def main() -> None:
    import torch

    from flink_jpmml_amd.bench import synth
    from flink_jpmml_amd.runtime.compiled import CompiledPmml
    from flink_jpmml_amd.runtime.plans import EPI_AFFINE

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "warmup": WARMUP, "repeat": REPEAT,
           "host_rows_timed": HOST_ROWS, "cases": {}}
    cases = [("naive_bayes_20x123", synth.naive_bayes_pmml(n_features=40, classes=20), True),
             ("softmax_40x200", document(200, 40, "softmax"), True),
             ("softmax_256x256", document(256, 256, "softmax"), True),
             ("softmax_256x256_no_probs", document(256, 256, "softmax"), False),
             ("regression_1x1024", document(1024, 0, "none"), False)]
    for name, text, with_probs in cases:
        c = CompiledPmml.from_string(text)
        outer = c.plan(dev)
        plan = getattr(outer, "inner", outer)
        assert plan.kind == "linear_wide", plan.kind
        K, F = plan.K, plan.n_features
        C = K if with_probs else 0
        X = torch.randn((ROWS, F), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(1))
        s, v = plan.alloc_outputs(ROWS)
        probs = torch.empty((ROWS, K), dtype=torch.float32, device=dev) if with_probs else None
        entry = {"tables": K, "fields": F, "probs": bool(with_probs),
                 "linear_wide_kernel": timed(lambda: plan.launch(X, s, v, probs=probs))}
        entry["linear_wide_kernel"].update(roofline(entry["linear_wide_kernel"]["median_ms"], F, K, C))
        W, b = plan.W[:F, :K].contiguous(), plan.b[:K].contiguous()

        def torch_path():
            y = torch.addmm(b, X, W)
            if plan.epi_args["mode"] == EPI_AFFINE:
                return y[:, 0], torch.isfinite(y[:, 0])
            p = torch.softmax(y, dim=1)
            return (p if with_probs else None), p.argmax(dim=1), torch.isfinite(p).all(dim=1)

        torch.backends.cuda.matmul.allow_tf32 = False
        entry["torch_addmm_and_epilogue"] = timed(torch_path)
        # the host oracle on the document's own inputs (the naive Bayes takes raw records, not design columns)
        Xh = synth.mixed_records(HOST_ROWS, 40, seed=3)[1].astype(np.float32) if outer is not plan \
            else X[:HOST_ROWS].cpu().numpy()
        t0 = time.perf_counter()
        so, vo = c.score_matrix_oracle(Xh, None, None)
        entry["host_oracle_seconds_per_million_rows"] = (time.perf_counter() - t0) * 1e6 / HOST_ROWS
        sd, vd = outer.score(Xh)
        agree = np.asarray(vo, bool) & vd.cpu().numpy()
        entry["host_compared"] = {"rows_valid_on_both": int(agree.sum()),
                                  "rows_with_another_validity": int((np.asarray(vo, bool) != vd.cpu().numpy()).sum())}
        if K > 1:
            entry["host_compared"]["rows_with_another_label"] = int(
                (sd.cpu().numpy()[agree] != np.asarray(so, np.float32)[agree]).sum())
        else:
            entry["host_compared"]["max_abs_difference"] = float(
                np.abs(sd.cpu().numpy()[agree].astype(np.float64) - np.asarray(so)[agree]).max())
        res["cases"][name] = entry
        del X, s, v, probs
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, ".")
    main()
