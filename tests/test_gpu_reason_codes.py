"""Scorecard reason codes on the MI355X: ``pmml_reasons_launch`` against its numpy twin bit for bit
(both code paths, both feature paths, every K, three input layouts, guarded outputs), and the public
routes against the host oracle's decoded codes on every row. Nothing here is rounded differently on
the two sides, so there are no tolerances."""

import numpy as np
import pytest

import _reason_cases as RC
from _reason_cases import CASES, bits

pytestmark = pytest.mark.gpu

GUARD = 7.0
ROW_COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
KERNEL_CASES = [c["name"] for c in CASES if c["kw"].get("use_reason_codes", True)]


@pytest.fixture(scope="module")
def lowered():
    """name -> (tables with an untouched column on either side, kernel matrix, valid, FieldPrep)."""
    out = {}
    for name in KERNEL_CASES:
        case = RC.CASE[name]
        _, plan = RC.dry_plan(RC.document(case))
        Xr, valid, prep = RC.kernel_inputs(plan, case["X"])
        T = plan.reasons
        cols = T.cols.copy()
        cols[:, 2] += 1
        out[name] = (RC.retabled(T, cols=cols, width=T.width + 2), Xr, valid, prep)
    return out


def _input(gpu, Xr, layout):
    """``Xr`` on the device: contiguous, rows padded to a multiple of four floats (the 16-byte loads
    and their tail), or an odd row stride from a base 4 bytes off a 16-byte boundary."""
    import torch

    m, F = Xr.shape
    if layout == "contiguous":
        return torch.from_numpy(Xr).to(gpu)
    ldx, off = ((F + 4) // 4 * 4, 0) if layout == "padded" else ((F + 1) | 1, 1)
    buf = torch.full((off + m * ldx + 3,), float("nan"), dtype=torch.float32, device=gpu)
    view = buf[off: off + m * ldx].view(m, ldx)[:, :F]
    view.copy_(torch.from_numpy(Xr).to(gpu))
    return view


def _launch(gpu, T, Xr, valid, prep, layout="contiguous", rows=None, feat_lds=None):
    import torch

    from flink_jpmml_amd.ops.reasons import reasons_launch

    m, W, pad = len(Xr), T.width, 3
    buf = torch.full((2 + m * (W + pad) + 2,), GUARD, dtype=torch.float32, device=gpu)
    out = buf[2: 2 + m * (W + pad)].view(m, W + pad)[:, :W]
    X = _input(gpu, Xr, layout)
    if layout == "odd":
        assert X.data_ptr() % 16 == 4 and X.stride(0) % 2 == 1
    vt = torch.from_numpy(valid).to(gpu)
    pt = torch.from_numpy(np.ascontiguousarray(prep).view(np.int32)).to(gpu) if prep is not None else None
    reasons_launch(X, vt, out, T, prep=pt, rows=rows, feat_lds=feat_lds)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _want(T, Xr, valid, prep):
    from flink_jpmml_amd.ops.reasons import reasons_numpy

    m, W, pad = len(Xr), T.width, 3
    buf = np.full(2 + m * (W + pad) + 2, GUARD, dtype=np.float32)
    body = np.full((m, W), GUARD, dtype=np.float32)
    reasons_numpy(Xr, valid, body, T, prep=prep)
    buf[2: 2 + m * (W + pad)].reshape(m, W + pad)[:, :W] = body
    assert (body[:, 0] == GUARD).all() and (body[:, -1] == GUARD).all()  # the untouched columns
    return buf


def _tile(a, m):
    return np.ascontiguousarray(a[np.arange(m) % len(a)])


def test_lds_bytes_match_the_library(gpu):
    from flink_jpmml_amd.ops import _lib
    from flink_jpmml_amd.ops.reasons import lds_bytes

    lib = _lib.load()
    for F in (1, 3, 9, 64, 300):
        for C in (1, 7, 64):
            for rows in (64, 128, 256):
                for shared in (0, 1):
                    for fl in (0, 1):
                        assert lib.pmml_reasons_lds_bytes(F, C, rows, shared, fl) == lds_bytes(F, C, rows, shared, fl)
    assert lib.pmml_reasons_lds_bytes(3, 65, 64, 1, 1) == -1 and lib.pmml_reasons_lds_bytes(3, 8, 96, 1, 1) == -1


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernel_equals_the_twin(gpu, lowered, name):
    """Every row count on the contiguous input with the lowering's geometry; at 129 and 257 rows also
    the padded and the odd-stride input, features from LDS and from global memory, and 64-row
    workgroups. The whole guarded buffer is compared: output columns, untouched columns, padding."""
    from flink_jpmml_amd.ops.reasons import LDS_BYTES, geometry, lds_bytes

    T, Xr, valid, prep = lowered[name]
    for m in ROW_COUNTS:
        X, v = _tile(Xr, m), _tile(valid, m)
        want = _want(T, X, v, prep)
        got = _launch(gpu, T, X, v, prep)
        assert np.array_equal(bits(got), bits(want)), (name, m)
        if m not in (129, 257):
            continue
        for layout in ("contiguous", "padded", "odd"):
            for feat_lds in (True, False):
                for rows in (geometry(T.n_feat, T.n_code, T.shared)[0], 64):
                    if lds_bytes(T.n_feat, T.n_code, rows, T.shared, feat_lds) > LDS_BYTES:
                        continue
                    got = _launch(gpu, T, X, v, prep, layout, rows, feat_lds)
                    assert np.array_equal(bits(got), bits(want)), (name, m, layout, feat_lds, rows)


def test_the_cases_cover_both_paths_and_every_k(lowered):
    from flink_jpmml_amd.ops.reasons import template_k

    seen = {(T.shared, template_k(T.k)) for T, _, _, _ in lowered.values()}
    assert seen == {(s, k) for s in (False, True) for k in (1, 2, 4, 8)}


def test_launch_checks_its_arguments(gpu, lowered):
    import torch

    from flink_jpmml_amd.ops.reasons import reasons_launch

    T, Xr, valid, _ = lowered["codes64_shared"]
    X, v = torch.from_numpy(Xr).to(gpu), torch.from_numpy(valid).to(gpu)
    out = torch.empty((len(Xr), T.width), dtype=torch.float32, device=gpu)
    for bad in (dict(X=X[:, :-1]), dict(out=out[:, :-1]), dict(valid=v[:5]), dict(rows=128), dict(rows=96)):
        kw = dict(X=X, valid=v, out=out, rows=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            reasons_launch(kw["X"], kw["valid"], kw["out"], T, rows=kw["rows"])


# --------------------------------------------------------------------------- public routes


def _csr(X):
    from flink_jpmml_amd.api.batch import SparseRecordBatch

    keep = ~np.isnan(X)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return SparseRecordBatch(indptr, np.nonzero(keep)[1].astype(np.int32), X[keep].astype(np.float32), X.shape[1])


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_routes_equal_the_host_oracle(gpu, name):
    import torch

    from flink_jpmml_amd.api.batch import BatchOutputs, RecordBatch
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.config import ScoringConfig

    case = RC.CASE[name]
    X = _tile(case["X"], max(300, len(case["X"])))
    text = RC.document(case)
    model = PmmlModel.from_string(text).bind(gpu, ScoringConfig(device=gpu, reason_codes=True, fallback="error"))
    assert model.on_device
    fields = [f"RC{r}" for r in case["kw"]["ranks"]]
    _, hv, host = model.predict_batch_outputs(X)
    want = {f: host.decode(f) for f in fields}
    if case["kw"].get("use_reason_codes", True):
        assert any(x is not None for x in want[fields[0]])

    def check(valid, outs, route):
        assert np.array_equal(np.asarray(valid, dtype=bool), hv), (name, route)
        for f in fields:
            assert outs.decode(f) == want[f], (name, route, f)

    s, v, outs = model.predict_batch_outputs(X, device=gpu, reason_codes=True)
    check(v.cpu().numpy(), outs, "predict_batch_outputs")
    pb = model.predict_records(RecordBatch(X), outputs=True)
    check(pb.valid, pb.outputs, "predict_records")
    pb = model.predict_records(_csr(X), outputs=True)
    check(pb.valid, pb.outputs, "sparse")
    plan = model.compiled.output_plan(gpu, reason_codes=True)
    Xt = torch.from_numpy(X).to(gpu)
    score, valid = plan.alloc_outputs(len(X))
    wide = plan.alloc_matrix(len(X))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    plan.launch(Xt, score, valid, stream=side, outputs=wide)  # every kernel of the plan on the side stream
    side.synchronize()
    check(valid.cpu().numpy(), BatchOutputs.from_wide(plan.names, wide, 0, model.compiled.schema, None), "side stream")


def test_default_scorer_still_refuses(gpu):
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.config import ScoringConfig
    from flink_jpmml_amd.runtime.plans import NotLowerable

    case = RC.CASE["equal_diffs"]
    strict = PmmlModel.from_string(RC.document(case)).bind(gpu, ScoringConfig(device=gpu, fallback="error"))
    with pytest.raises(NotLowerable) as e:
        strict.predict_records(RecordBatch(case["X"]), outputs=True)
    assert "RC1" in str(e.value)
