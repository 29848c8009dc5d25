"""Radial-basis-function networks on the device: ``rbf_kernel`` (``ops/csrc/rbf.hip``) against the
same arithmetic as torch tensor ops on the same GPU, and the host oracle on a row sample.

Two synthetic networks (``bench/synth.py::rbf_pmml``) over 1M standard-normal fp32 rows resident in HBM:

* ``reg64x256``: 64 inputs, 256 units, one regression output, no hidden normalisation;
* ``cls32x1024``: 32 inputs, 1024 units, 8 classes, ``simplemax`` hidden layer.

The torch formulation: input affine map, the expansion ``|x|^2 - 2 x W^T + |w|^2`` with ``addmm``,
``exp``, the row normalisation and ``addmm`` for the output layer (softmax + argmax for the
classifier), fp32, in row chunks that bound the ``[rows, units]`` matrix. Timed with device events
over ``REPEAT`` rounds after ``WARMUP``, the two alternated launch by launch; medians are reported.
Run from the repository root on a machine with a GPU::

    PYTHONPATH=. python profiles/rbf/measure.py [rows] > results.json
"""

import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = 2_000  # the oracle loops over the units in Python: timed on a slice
WARMUP, REPEAT = 3, 10
CHUNK = 1 << 18

MODELS = {
    "reg64x256": dict(n_features=64, hidden=256, n_out=1, seed=1),
    "cls32x1024": dict(n_features=32, hidden=1024, n_out=8, seed=1, classification=True, normalization="simplemax"),
}


def torch_twin(plan, c):
    """The plan's network as torch ops on the plan's device (unpermuted fp32 operands)."""
    import torch

    from flink_jpmml_amd.runtime.nn_plans import _affine_of

    rbf = c.evaluator.rbf_layers()
    dev = plan.device
    maps = np.array([_affine_of(i.derived.expression)[:2] for i in c.evaluator.nn.inputs])
    sc, sh = (torch.tensor(maps[:, k], dtype=torch.float32, device=dev) for k in (0, 1))
    Wt = torch.tensor(rbf["centers"].T, dtype=torch.float32, device=dev).contiguous()
    wn = (Wt * Wt).sum(0)
    cj = torch.tensor(rbf["fan_in"] * np.log(rbf["altitude"]), dtype=torch.float32, device=dev)
    gj = torch.tensor(1.0 / (2.0 * rbf["width"] ** 2), dtype=torch.float32, device=dev)
    V, b = (torch.tensor(a, dtype=torch.float32, device=dev) for a in rbf["output"][:2])
    simplemax, cls = rbf["normalization"] == "simplemax", plan.is_classification

    def run(X, score):
        for lo in range(0, X.shape[0], CHUNK):
            x = X[lo: lo + CHUNK] * sc + sh
            d = torch.addmm(wn, x, Wt, alpha=-2.0) + (x * x).sum(1, keepdim=True)
            a = torch.exp(cj - gj * d.clamp_min_(0.0))
            if simplemax:
                a = a / a.sum(1, keepdim=True)
            o = torch.addmm(b, a, V)
            score[lo: lo + CHUNK] = torch.softmax(o, 1).argmax(1).float() if cls else o[:, 0]

    return run


def main() -> None:
    import torch

    from flink_jpmml_amd.bench import synth
    from flink_jpmml_amd.runtime.compiled import CompiledPmml

    out = {"rows": ROWS, "device": torch.cuda.get_device_name(0)}
    for name, kw in MODELS.items():
        c = CompiledPmml.from_string(synth.rbf_pmml(**kw))
        plan = c.plan("cuda")
        X = torch.from_numpy(synth.stream_matrix(ROWS, kw["n_features"], seed=7)).cuda()
        s, v = plan.alloc_outputs(ROWS)
        s2 = torch.empty_like(s)
        twin = torch_twin(plan, c)
        fns = {"kernel_ms": lambda: plan.launch(X, s, v), "torch_ms": lambda: twin(X, s2)}
        for _ in range(WARMUP):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(REPEAT):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        res = {k: float(np.median(t)) for k, t in ms.items()}
        res["agree"] = float((s == s2).float().mean()) if plan.is_classification else float((s - s2).abs().max())
        flops = 2.0 * ROWS * plan.n_tiles * 32 * (plan.kp + 32)  # both products, padded
        res["kernel_tflops_fp32_mfma"] = flops / res["kernel_ms"] / 1e9
        Xh = X[:HOST_ROWS].cpu().numpy()
        t0 = time.perf_counter()
        c.score_matrix_oracle(Xh)
        res["host_oracle_us_per_row"] = (time.perf_counter() - t0) / HOST_ROWS * 1e6
        out[name] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
