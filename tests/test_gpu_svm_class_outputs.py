"""Class outputs of SVM classifiers on the MI355X: the class-output instantiations of ``svm.hip``
through ``SvmPlan`` / ``SvmWidePlan`` / ``SvmGemmPlan.launch(probs=)``, ``OutputPlan(svm_classes=True)``
and the public routes. The exact documents (``_svm_vote_cases``: integer data, linear kernels) match the
float64 reference in every bit: vote counts are integers and a share is one IEEE division. The
polynomial / RBF / sigmoid documents match the oracle in every bit on the rows on which every machine's
decision value is further from its threshold than twice the bound ``tests/test_gpu_exact.py`` pins."""

import numpy as np
import pytest

import _exact as E
import _svm_vote_cases as SC
from _exact import strided
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.models.base import class_probabilities
from flink_jpmml_amd.runtime.outputs import oracle_outputs, oracle_top_k

pytestmark = pytest.mark.gpu

GUARD = 7.0
ROW_COUNTS = (1, 33, 255, 256, 257, 513)
TOP = 3


def _base(plan):
    while getattr(plan, "inner", None) is not None:
        plan = plan.inner
    return plan


def _expect_path(c, base):
    """The kernel a case is meant to reach."""
    name = type(base).__name__
    assert name == c.plan, (c.name, name)
    if name == "SvmPlan":
        assert (base.n_svp >= 32) == (c.n_sv >= 32), c.name  # < 32 support vectors: the VALU kernel
    if c.name == "mfma-32sv":
        assert base.n_machines == 1 and base.n_svp == 32  # the NM = 1 instantiation
    if c.name in ("mfma-33sv", "mfma-65sv", "m8c16", "oaa-noalt"):
        assert base.n_machines > 1 and base.n_svp >= 32
    if c.name == "wide-17cls":
        assert base.n_machines == 136 and base.n_groups > 1
    if c.name == "m128c256":
        assert base.n_classes == 256 and base.n_machines == 128


@pytest.mark.parametrize("name", SC.ALL_NAMES)
def test_exact_documents(gpu, name):
    """Raw index / validity / shares of the index-mode plan, every column and the top-3 of the output
    plan, and its score against the scoring plan, for every row count."""
    import torch

    c = SC.case(name)
    compiled = PmmlModel.from_string(c.pmml(SC.class_outputs(c))).compiled
    plan = compiled.output_plan(gpu, svm_classes=True, top_k=TOP, svm_impl=c.impl)
    inner, base = plan.inner, _base(plan.inner)
    assert base.table is None
    _expect_path(c, base)
    scoring = compiled.plan(gpu, svm_impl=c.impl)
    assert _base(scoring).table is not None
    C = c.n_classes
    Xall = SC.rows(c, max(ROW_COUNTS))
    s, v, cols, res, ok = oracle_outputs(compiled, Xall, top_k=TOP)
    lab, valid, shares, total = SC.reference(c, Xall)
    want = SC.expected_columns(c, compiled.schema, Xall)
    ti, tp = oracle_top_k(class_probabilities(res), valid, TOP)
    if name in SC.NO_VOTE_CASES:
        assert (valid & (total == 0)).any()
    for n in ROW_COUNTS:
        X = torch.from_numpy(Xall[:n]).to(gpu)
        raw_s, raw_v = inner.alloc_outputs(n)
        probs = torch.full((n, C), GUARD, dtype=torch.float32, device=gpu)
        inner.launch(X, raw_s, raw_v, probs=probs)
        sc, va, mat = plan.score_outputs(Xall[:n])
        s0, v0 = scoring.score(Xall[:n])
        torch.cuda.synchronize()
        assert np.array_equal(raw_v.cpu().numpy() != 0, valid[:n]), (name, n)
        assert np.array_equal(SC.bits(raw_s.cpu().numpy()), SC.bits(lab[:n])), (name, n)
        assert np.array_equal(SC.bits(probs.cpu().numpy()), SC.bits(shares[:n])), (name, n)
        mat = mat.cpu().numpy()
        for i, col in enumerate(plan.names):
            assert np.array_equal(SC.bits(mat[:, i]), SC.bits(want[col][:n])), (name, n, col)
            assert np.array_equal(SC.bits(mat[:, i]), SC.bits(cols[col][:n])), (name, n, col)
        w = len(plan.names)
        assert np.array_equal(np.nan_to_num(mat[:, w: w + TOP], nan=-1).astype(np.int64), ti[:n]), (name, n)
        assert np.array_equal(SC.bits(mat[:, w + TOP:]), SC.bits(tp[:n])), (name, n)
        # the output plan's score and validity are the scoring plan's (a string target: EmptyScore on both)
        assert np.array_equal(SC.bits(sc.cpu().numpy()), SC.bits(s0.cpu().numpy())), (name, n)
        assert np.array_equal(va.cpu().numpy() != 0, v0.cpu().numpy() != 0), (name, n)
        assert np.array_equal(SC.bits(sc.cpu().numpy()), SC.bits(s[:n])), (name, n)
        if c.target_type != "string":
            assert np.array_equal(va.cpu().numpy() != 0, valid[:n]), (name, n)
        else:
            assert not va.cpu().numpy().any()


@pytest.mark.parametrize("name", ["valu-31sv", "mfma-33sv", "wide-5cls", "wide-17cls", "oaa-noalt-wide"])
def test_layouts_guards_and_a_side_stream(gpu, name):
    """A contiguous input and a column view of a wider matrix; ``outputs`` a view with guard columns and
    guard elements around it; ``probs`` between guard rows (C odd: its base is not 16-byte aligned);
    the launches on a side stream."""
    import torch

    c = SC.case(name)
    C = c.n_classes
    assert C % 2 == 1
    compiled = PmmlModel.from_string(c.pmml(SC.class_outputs(c))).compiled
    plan = compiled.output_plan(gpu, svm_classes=True, top_k=TOP, svm_impl=c.impl)
    n, W, pad = 261, plan.width, 3
    Xn = SC.rows(c, n)
    _, _, cols, res, ok = oracle_outputs(compiled, Xn, top_k=TOP)
    lab, valid, shares, _ = SC.reference(c, Xn)
    side = torch.cuda.Stream(device=gpu)
    for layout in ("contiguous", "view"):
        Xt = torch.from_numpy(Xn).to(gpu) if layout == "contiguous" else \
            torch.from_numpy(strided(Xn)).to(gpu)[:, : Xn.shape[1]]
        buf = torch.full((2 + n * (W + pad) + 2,), GUARD, dtype=torch.float32, device=gpu)
        out = buf[2: 2 + n * (W + pad)].view(n, W + pad)[:, :W]
        score, vout = plan.alloc_outputs(n)
        pbuf = torch.full((n + 2, C), GUARD, dtype=torch.float32, device=gpu)
        raw_s, raw_v = plan.inner.alloc_outputs(n)
        torch.cuda.synchronize()
        plan.launch(Xt, score, vout, stream=side, outputs=out)
        plan.inner.launch(Xt, raw_s, raw_v, stream=side, probs=pbuf[1: n + 1])
        side.synchronize()
        host = buf.cpu().numpy()
        body = host[2: 2 + n * (W + pad)].reshape(n, W + pad)
        assert (host[:2] == GUARD).all() and (host[-2:] == GUARD).all() and (body[:, W:] == GUARD).all(), layout
        for i, col in enumerate(plan.names):
            assert np.array_equal(SC.bits(body[:, i]), SC.bits(cols[col])), (layout, col)
        p = pbuf.cpu().numpy()
        assert (p[0] == GUARD).all() and (p[-1] == GUARD).all(), layout
        assert np.array_equal(SC.bits(p[1:-1]), SC.bits(shares)), layout
        assert np.array_equal(SC.bits(raw_s.cpu().numpy()), SC.bits(lab)), layout
        assert np.array_equal(raw_v.cpu().numpy() != 0, valid), layout


INEXACT = [(n, k) for n in E.NONLINEAR_SVM_CASES if E.SVM_CASES[n][2] >= 2  # a regression SVM has no classes
           for k in ("polynomial", "radialBasis", "sigmoid")]


@pytest.mark.parametrize("name,kernel", INEXACT)
def test_inexact_kernels_on_decided_rows(gpu, name, kernel):
    """Label and shares equal the oracle's in every bit wherever every machine's oracle decision value
    is further from its threshold than ``2 * SVM_ULP_CONSTANT * 2^-24 * T``; those rows are at least
    90 % of the valid rows (largest share left out: 33 of 499, wide-9cls polynomial)."""
    c = SC.ProbeCase(name, kernel=kernel)
    compiled = PmmlModel.from_string(c.pmml(SC.class_outputs(c))).compiled
    X = E.svm_matrix(E.SVM_ROWS, c.F, seed=6)
    valid = ~np.isnan(X).any(axis=1)
    decided = SC.decided_rows(c.probe, X)
    print(name, kernel, "left out", int((valid & ~decided).sum()), "of", int(valid.sum()))
    assert (valid & decided).sum() >= 0.9 * valid.sum()
    s, v, cols, res, ok = oracle_outputs(compiled, X, top_k=TOP)
    plan = compiled.output_plan(gpu, svm_classes=True, top_k=TOP, svm_impl=c.impl)
    assert type(_base(plan.inner)).__name__ == c.plan
    sc, va, mat = plan.score_outputs(X)
    sc, va, mat = sc.cpu().numpy(), va.cpu().numpy() != 0, mat.cpu().numpy()
    keep = decided | ~valid
    assert np.array_equal(va, v)
    assert np.array_equal(SC.bits(sc[keep]), SC.bits(s[keep]))
    for i, col in enumerate(plan.names):
        assert np.array_equal(SC.bits(mat[keep, i]), SC.bits(cols[col][keep])), (name, kernel, col)
    ti, tp = oracle_top_k(class_probabilities(res), valid, TOP)
    w = len(plan.names)
    assert np.array_equal(np.nan_to_num(mat[keep, w: w + TOP], nan=-1).astype(np.int64), ti[keep])
    assert np.array_equal(SC.bits(mat[keep, w + TOP:]), SC.bits(tp[keep]))


@pytest.mark.parametrize("impl", ["fused", "wide"])
def test_launcher_rejects_what_it_cannot_take(gpu, impl, monkeypatch):
    """Past the plans' own checks: a classification launch with neither a table nor ``probs``, and
    ``probs`` with a regression model, end in the launcher with -4 before any kernel runs."""
    import torch

    from flink_jpmml_amd.bench import synth
    from flink_jpmml_amd.runtime import nn_plans

    cls = _base(PmmlModel.from_string(SC.case("m8c16").pmml()).compiled.plan(gpu, svm_impl=impl))
    reg = _base(PmmlModel.from_string(synth.svm_pmml(8, 40, classification=False)).compiled.plan(gpu, svm_impl=impl))
    X = torch.zeros((5, 8), device=gpu)
    s, v = cls.alloc_outputs(5)
    with pytest.raises(ValueError, match="no class vote shares"):
        reg.launch(X, s, v, probs=torch.zeros((5, 16), device=gpu))
    with pytest.raises(ValueError, match="contiguous"):
        cls.launch(X, s, v, probs=torch.zeros((5, 32), device=gpu)[:, ::2])
    cls.table = None
    with pytest.raises(ValueError, match="needs probs"):
        cls.launch(X, s, v)
    monkeypatch.setattr(nn_plans, "_svm_probs", lambda plan, X, probs, C: None if probs is None else probs.data_ptr())
    with pytest.raises(Exception, match="-4"):
        cls.launch(X, s, v)
    with pytest.raises(Exception, match="-4"):
        reg.launch(X, s, v, probs=torch.zeros((5, 16), device=gpu))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["str-ovo3", "oaa-noalt-wide", "gemm-m9c18"])
def test_public_routes(gpu, name):
    """``predict_batch_outputs(svm_classes=True)`` and ``ScoringConfig(svm_classes=True,
    fallback="error")`` through ``predict_records(outputs=True)``: the host's columns and label strings."""
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.config import ScoringConfig

    c = SC.case(name)
    text = c.pmml(SC.class_outputs(c))
    X = SC.rows(c, 70)
    opts = {} if c.impl == "auto" else {"svm_impl": c.impl}
    model = PmmlModel.from_string(text)
    hs, hv, host = model.predict_batch_outputs(X, top_k=TOP)
    s, v, outs = model.predict_batch_outputs(X, device=gpu, svm_classes=True, top_k=TOP, **opts)
    assert np.array_equal(v.cpu().numpy() != 0, hv)
    outs = outs.numpy()
    for n in outs.names:
        assert np.array_equal(SC.bits(outs[n]), SC.bits(host[n])), n
    labels = host.decode("lab")
    assert outs.decode("lab") == labels and None in labels and c.categories[0] in labels
    assert np.array_equal(np.asarray(outs.top_index), host.top_index)
    assert np.array_equal(SC.bits(outs.top_probability), SC.bits(host.top_probability))
    if c.impl != "auto":
        return  # ScoringConfig takes the plan compile_plan picks
    bound = PmmlModel.from_string(text).bind(gpu, ScoringConfig(device=gpu, svm_classes=True, fallback="error"))
    assert bound.on_device
    pb = bound.predict_records(RecordBatch(X), outputs=True)
    assert np.array_equal(np.asarray(pb.valid, dtype=bool), hv)
    assert pb.outputs.decode("lab") == labels
    served = pb.outputs.numpy()
    for n in ("pwin", "p_nobody", outs.names[3]):
        assert np.array_equal(SC.bits(served[n]), SC.bits(host[n])), n
    strict = PmmlModel.from_string(text).bind(gpu, ScoringConfig(device=gpu, fallback="error"))
    with pytest.raises(Exception, match="output 'lab': SvmPlan has no index mode"):  # off: refused by name
        strict.predict_records(RecordBatch(X), outputs=True)
