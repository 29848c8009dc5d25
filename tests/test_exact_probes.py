"""The exact-integer probes of ``tests/_exact.py`` are exact and sensitive (CPU).

For every family and shape that ``tests/test_gpu_exact.py`` runs on the device, with plans lowered
under ``lowering_dry_run()``: the dense float64 reference, the float64 oracle and the numpy twin of
the kernel over the plan's packed tensors agree in every bit (validity included), the exactness
guard holds, and every named mutant of the packed tensors changes at least one compared bit — a
mutant no row detects means the probes are too weak, not that the kernel is right."""

import numpy as np
import pytest
import torch

import _exact as E
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.nn_plans import MlpPlan, SvmPlan, WideMlpPlan
from flink_jpmml_amd.runtime.plans import ClusterPlan, KnnPlan, compile_plan, lowering_dry_run
from test_cluster_mfma import _emulate_mfma
from test_knn import _emulate_knn_kernel
from test_svm_wide import emulate as emulate_svm_wide
from test_svm_wide import finish as finish_svm
from test_wide_mlp import _bf16, emulate_wide

def _plan(c, **kw):
    with lowering_dry_run():
        return compile_plan(c, torch.device("cpu"), **kw)


def _same(a, b) -> bool:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(E.bits(a), E.bits(b)) and np.array_equal(np.isnan(a), np.isnan(b))


def _oracle_rows(n: int, step: int) -> np.ndarray:
    """A fixed subsample for the per-connection network oracle."""
    return np.unique(np.concatenate([np.arange(0, n, step), np.arange(min(n, 40))]))


# --------------------------------------------------------------------------- fused MLP twin


def unpack_fused(plan: MlpPlan):
    """``[(Wt [units, k], bias [units])]`` (padded) of an MlpPlan's packed A fragments, un-permuted
    with mlp.hip's index map: fragment (tile t, k-step s, lane, j) is unit ``32 t + (lane & 31)`` and,
    with h = lane >> 5, B-operand k ``16 s + 8 h + j`` (bf16, first layer), ``32 (s >> 1) + 16 (s & 1)
    + 8 (j >> 2) + 4 h + (j & 3)`` (bf16, later layers: the previous accumulator registers),
    ``2 s + h`` (fp32, first) or ``32 (s >> 4) + (r & 3) + 8 (r >> 2) + 4 h`` with r = s & 15 (fp32, later)."""
    w = plan.weights.float().numpy()
    B = plan.biases.numpy()
    lm = plan.layer_meta.numpy()
    per, kstep = (8, 16) if plan.bf16 else (1, 2)
    out = []
    for L in range(plan.n_layers):
        kp, mp, mreal, wo, bo, act = (int(v) for v in lm[L, :6])
        assert act in (0, 3)
        ks, mt = kp // kstep, mp // 32
        fr = w[wo: wo + mt * ks * 64 * per].reshape(mt, ks, 64, per)
        Wt = np.zeros((mp, kp), np.float32)
        for s in range(ks):
            for lane in range(64):
                h, r = lane >> 5, lane & 31
                for j in range(per):
                    if plan.bf16:
                        k = 16 * s + 8 * h + j if L == 0 else \
                            32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3)
                    else:
                        q = s & 15
                        k = 2 * s + h if L == 0 else 32 * (s >> 4) + (q & 3) + 8 * (q >> 2) + 4 * h
                    Wt[r::32, k][: mt] = fr[:, s, lane, j]
        out.append((Wt, B[bo: bo + mp].copy()))
    return out


def emulate_fused(plan: MlpPlan, X, logits: bool = False):
    """numpy model of mlp.hip over the packed A fragments (``unpack_fused``): bf16 or fp32 operands,
    fp32 accumulation, activations rounded to the operand type between layers. ``logits``: the
    output neurons' values instead of the decoded score."""
    X = np.asarray(X, np.float32)
    x = X[:, plan.in_index.numpy()]
    sc, sh, ms = (t.numpy() for t in (plan.in_scale, plan.in_shift, plan.in_missing))
    z = np.where(np.isnan(x), ms, x * sc + sh)
    ok = ~np.isnan(z).any(axis=1)
    rnd = _bf16 if plan.bf16 else (lambda a: np.asarray(a, np.float32))
    H = np.zeros((len(X), plan.k0), np.float32)
    H[:, : plan.n_in] = np.nan_to_num(z)
    H = rnd(H)
    packed = unpack_fused(plan)
    for L, (Wt, b) in enumerate(packed):
        Z = (H[:, : Wt.shape[1]].astype(np.float64) @ Wt.T.astype(np.float64)).astype(np.float32) + b
        H = Z if L == len(packed) - 1 else rnd(np.maximum(Z, 0))
    out = H[:, : plan.n_out]
    if logits:
        return np.where(ok[:, None], out.astype(np.float64), np.nan), ok
    s = plan.table.numpy()[out.argmax(1)].astype(np.float64) if plan.is_classification \
        else plan.out_a * out[:, 0].astype(np.float64) + plan.out_b
    return np.where(ok, s, np.nan), ok


def _check_network(name, shape, seed, precision, cls_expected, twin, norm="softmax"):
    layers, cls, doc = E.network(shape, seed, norm)
    c = CompiledPmml.from_string(doc)
    plan = _plan(c, precision=precision)
    assert isinstance(plan, cls_expected), type(plan)
    n_in = shape["n_in"]
    X = E.probe_matrix(E.nn_rows(n_in), n_in, seed=seed)
    ref, vref, logits = E.nn_reference(layers, X, cls)  # asserts the exactness guard
    s, v = twin(plan, X)
    assert np.array_equal(v, vref) and _same(s, ref), name
    idx = _oracle_rows(len(X), 1 if len(layers[0][0]) * layers[0][0].shape[1] < 40_000 else 9)
    so, vo = c.score_matrix_oracle(X[idx])
    assert np.array_equal(vo, vref[idx]) and _same(so, ref[idx]), name
    if cls:
        assert E.tie_rows(logits)[vref].any()
        if norm is None:  # the oracle's class outputs are the integer logits
            assert np.array_equal(c.result(X[idx]).probs[vo], logits[idx][vo])
    return plan, X, ref


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", list(E.FUSED_SHAPES) + list(E.WIDE_SHAPES))
def test_network_probe_sees_every_stored_parameter(name, which):
    """Every non-zero weight of every layer and every bias changes a compared output (the
    regression value, or the logits that ``probs=`` returns without normalisation) on some row."""
    shape, seed = E.FUSED_SHAPES.get(name) or E.WIDE_SHAPES[name], E.seeds(name)[which]
    layers = E.int_network(seed=seed, **shape)
    X = E.probe_matrix(E.nn_rows(shape["n_in"]), shape["n_in"], seed=seed)
    assert E.nn_insensitive(layers, X) == []
    # and a zero position a kernel filled wrongly would show: its input is set on a row with the unit active
    assert E.nn_blind_positions(layers, X) == []


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", list(E.FUSED_SHAPES))
def test_fused_mlp_probe_twin_equals_oracle(name, which, precision):
    seed = E.seeds(name)[which]
    for norm in E.norms(E.FUSED_SHAPES[name]):
        _check_network(name, E.FUSED_SHAPES[name], seed, precision, MlpPlan, emulate_fused, norm)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", list(E.WIDE_SHAPES))
def test_wide_mlp_probe_twin_equals_oracle_and_mutants_show(name, which, precision):
    seed = E.seeds(name)[which]
    shape = E.WIDE_SHAPES[name]
    for norm in E.norms(shape):
        plan, X, ref = _check_network(name, shape, seed, precision, WideMlpPlan, emulate_wide, norm)
    layers, cls, _ = E.network(shape, seed)
    if cls:  # labels are coarse: the mutants are judged on the first class's integer logit
        plan.is_classification, ref = False, E.nn_reference(layers, X, True)[2][:, 0]
        ref = np.where(np.isnan(X).any(axis=1), np.nan, ref)
        assert _same(emulate_wide(plan, X)[0], ref)
    W0, B0 = plan.wts.float().numpy().copy(), plan.bss.numpy().copy()
    for mname, mutate in E.wide_mutants(plan.dims, shape["n_in"], layers).items():
        W, B = W0.copy(), B0.copy()
        mutate(W, B)
        plan.wts, plan.bss = torch.from_numpy(W).to(plan._dtype()), torch.from_numpy(B)
        s, _ = emulate_wide(plan, X)
        assert not _same(s, ref), f"{name}: mutant {mname} changes no output bit"
    plan.wts, plan.bss = torch.from_numpy(W0).to(plan._dtype()), torch.from_numpy(B0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", list(E.FUSED_SHAPES))
def test_fused_mlp_mutants_show(name, which, precision):
    """Every named mutant (``_exact.layer_mutants``) of every layer of the fused kernel's packed A
    fragments: the fragments are un-permuted with the kernel's index map, the logical (unit, k) or
    bias position is altered, the layers are packed again, and the twin over the new fragments must
    differ from the reference in a compared bit (the regression value, or the integer logits)."""
    from flink_jpmml_amd.runtime.nn_plans import pack_mlp_weights

    shape, seed = E.FUSED_SHAPES[name], E.seeds(name)[which]
    layers, cls, doc = E.network(shape, seed, None)
    plan = _plan(CompiledPmml.from_string(doc), precision=precision)
    X = E.probe_matrix(E.nn_rows(shape["n_in"]), shape["n_in"], seed=seed)
    ok = ~np.isnan(X).any(axis=1)
    ref = np.where(ok[:, None], E.nn_reference(layers, X, cls)[2], np.nan)
    clean = unpack_fused(plan)

    def run(packed):
        w, b, meta = pack_mlp_weights([(Wt.T, bias) for Wt, bias in packed], "bf16" if plan.bf16 else "fp32")
        assert [m[:2] for m in meta] == [Wt.shape[::-1] for Wt, _ in packed]
        wt = torch.from_numpy(w.astype(np.float32))
        plan.weights, plan.biases = (wt.to(torch.bfloat16) if plan.bf16 else wt), torch.from_numpy(b.astype(np.float32))
        return emulate_fused(plan, X, logits=True)[0]

    assert _same(run(clean), ref)  # unpack and pack are inverse, and the twin equals the reference
    for L, (W, _) in enumerate(layers):
        for mname, mutate in E.layer_mutants(*W.shape).items():
            packed = [(Wt.copy(), b.copy()) for Wt, b in clean]
            mutate(*packed[L])
            assert not _same(run(packed), ref), f"{name}: layer {L} mutant {mname} changes no output bit"


# --------------------------------------------------------------------------- SVM


def emulate_svm(plan: SvmPlan, X):
    """numpy model of svm.hip's fused kernels over SvmPlan's padded tensors (linear kernel)."""
    X = np.asarray(X, np.float32)
    xb = np.zeros((len(X), plan.fmax), np.float64)
    xb[:, : plan.n_in] = X[:, plan.in_index.numpy()]
    bad = np.isnan(xb).any(1)
    G = np.nan_to_num(xb) @ plan.sv.numpy().astype(np.float64).T
    D = G @ plan.coef.numpy().astype(np.float64) + plan.intercept.numpy()
    return D[:, : plan.n_machines], bad


@pytest.mark.parametrize("name", list(E.SVM_CASES))
def test_svm_probe_twin_equals_oracle(name):
    p, kind = E.svm_probe(name)
    c = CompiledPmml.from_string(p.pmml())
    plan = _plan(c)
    assert type(plan).__name__ == kind
    X = E.svm_matrix(E.SVM_ROWS, p.F)
    ref, vref, D = p.reference(X)
    assert np.array_equal(c.evaluator.decision_values(np.nan_to_num(X.astype(np.float64))), D)
    so, vo = c.score_matrix_oracle(X)
    assert np.array_equal(vo, vref) and _same(so, ref)
    Dk, bad = (emulate_svm if kind == "SvmPlan" else emulate_svm_wide)(plan, X)
    assert np.array_equal(~bad, vref) and np.array_equal(E.bits(Dk), E.bits(D))
    s, v = finish_svm(plan, Dk, bad)
    assert _same(s, ref)
    if p.n_classes >= 2:
        assert ((D == 0).any(axis=1) & vref).mean() >= 0.01  # decision values exactly on the threshold
    # every support-vector entry and every dual coefficient moves a decision value on some valid row
    # (D = X S^T A + b): every field is non-zero on a row, every vector has a coefficient, every
    # vector's product with some row is non-zero; an intercept moves its whole column
    Xv = np.asarray(X, np.float64)[vref]
    assert (Xv != 0).any(axis=0).all() and (p.A != 0).any(axis=1).all() and ((Xv @ p.S.T) != 0).any(axis=0).all()

    # mutants of the packed dual coefficients / machines
    def differs(Dm):
        return not np.array_equal(E.bits(Dm), E.bits(D))

    if kind == "SvmPlan" and p.n_sv > 4:
        for d in (4, 32):
            if p.n_sv > d:
                A0 = plan.coef.numpy().copy()
                A = A0.copy()
                A[[0, d]] = A0[[d, 0]]
                plan.coef = torch.from_numpy(A)
                assert differs(emulate_svm(plan, X)[0]), f"swap dual coefficients j, j + {d}"
                plan.coef = torch.from_numpy(A0)
    if kind == "SvmWidePlan" and p.n_sv > 4:
        A0 = plan.coefA.numpy().copy()  # [tile, mtile, lane, register]
        A = A0.copy()
        A[0, :, :32, 0], A[0, :, 32:, 0] = A0[0, :, 32:, 0], A0[0, :, :32, 0]  # vectors p(0, 0) = 0 and p(0, 1) = 4
        plan.coefA = torch.from_numpy(A)
        assert differs(emulate_svm_wide(plan, X)[0]), "swap dual coefficients j, j + 4"
        if p.n_sv > 32:
            A = A0.copy()
            A[0, :, :, 0], A[1, :, :, 0] = A0[1, :, :, 0], A0[0, :, :, 0]
            plan.coefA = torch.from_numpy(A)
            assert differs(emulate_svm_wide(plan, X)[0]), "swap dual coefficients j, j + 32"
        if plan.n_machines > 33:
            A = A0.copy()
            A[:, 0, 1], A[:, 1, 1] = A0[:, 1, 1], A0[:, 0, 1]  # machines 1 and 33 (lane 1 of tiles 0 / 1)
            plan.coefA = torch.from_numpy(A)
            assert differs(emulate_svm_wide(plan, X)[0]), "swap machines m, m + 32"
        plan.coefA = torch.from_numpy(A0)


@pytest.mark.parametrize("kernel", ["polynomial", "radialBasis", "sigmoid"])
@pytest.mark.parametrize("name", E.NONLINEAR_SVM_CASES)
def test_nonlinear_svm_bound_separates_a_swapped_coefficient_pair(name, kernel):
    """The kernels that are not exact are compared on the device against a bound that scales with
    every entry (``_exact.SVM_ULP_CONSTANT`` times 2^-24 times ``kernel_terms``' T). The
    float64 twin over the packed tensors sits far inside it, and with one pair of dual coefficients
    swapped far outside: the probe coefficients are large enough for the bound to see a swap."""
    p, kind = E.svm_probe(name, kernel=kernel)
    c = CompiledPmml.from_string(p.pmml())
    plan = _plan(c)
    assert type(plan).__name__ == kind
    X = E.svm_matrix(300, p.F, seed=6)
    X = X[~np.isnan(X).any(axis=1)]
    D, T = p.kernel_terms(X)
    np.testing.assert_allclose(c.evaluator.decision_values(X.astype(np.float64)), D, rtol=1e-12, atol=1e-12)
    bound = E.SVM_ULP_CONSTANT * 2.0 ** -24 * T

    def twin():
        if kind == "SvmWidePlan":
            return emulate_svm_wide(plan, X)[0]
        xb = np.zeros((len(X), plan.fmax))
        xb[:, : plan.n_in] = X[:, plan.in_index.numpy()]
        S, A = plan.sv.numpy().astype(np.float64), plan.coef.numpy().astype(np.float64)
        G = xb @ S.T
        if kernel == "radialBasis":
            K = np.exp(-plan.gamma * np.maximum((xb * xb).sum(1)[:, None] - 2 * G + plan.sv_norm.numpy()[None], 0))
        elif kernel == "polynomial":
            K = (plan.gamma * G + plan.coef0) ** plan.degree
        else:
            K = np.tanh(plan.gamma * G + plan.coef0)
        return (K @ A + plan.intercept.numpy())[:, : plan.n_machines]

    assert (np.abs(twin() - D) <= 0.01 * bound).all()
    if kind == "SvmWidePlan":
        A0 = plan.coefA.numpy().copy()
        A = A0.copy()
        A[0, :, :32, 0], A[0, :, 32:, 0] = A0[0, :, 32:, 0], A0[0, :, :32, 0]
        plan.coefA = torch.from_numpy(A)
    else:
        A0 = plan.coef.numpy().copy()
        A = A0.copy()
        A[[0, 4]] = A0[[4, 0]]
        plan.coef = torch.from_numpy(A)
    assert (np.abs(twin() - D) > bound).any()


# --------------------------------------------------------------------------- clustering


@pytest.mark.parametrize("metric", ["squaredEuclidean", "euclidean", "cityBlock", "chebychev"])
@pytest.mark.parametrize("K,F", E.CLUSTER_CASES)
def test_cluster_probe_reference_equals_oracle(K, F, metric):
    C, w = E.grid_centers(K, F, seed=K), E.field_weights(F, seed=F)
    c = CompiledPmml.from_string(E.cluster_pmml(C, w, metric))
    X = E.center_matrix(C, 513, seed=K + F)  # row 16: no field present, no prediction
    label, aff, ok, raw = E.cluster_reference(C, w, X, metric)
    if metric == "squaredEuclidean":
        assert E.centers_insensitive(C, w, X) == []
    so, vo = c.score_matrix_oracle(X)
    assert np.array_equal(vo, ok) and np.array_equal(so[ok], label[ok] + 1.0)
    assert E.min_tie_rows(raw)[ok].any()
    full = ~np.isnan(X).any(axis=1)
    res = c.result(X)
    assert np.array_equal(res.affinity[full], aff[full])
    np.testing.assert_allclose(res.affinity[ok], aff[ok], rtol=1e-15)
    if metric in ("squaredEuclidean", "euclidean"):
        plan = _plan(c, cluster_variant="mfma")
        assert isinstance(plan, ClusterPlan) and plan.variant == "mfma"
        wc, cc = plan.wc.numpy(), plan.cc.numpy()
        k, a = _emulate_mfma(wc, cc, w, X[full], metric == "euclidean")
        assert np.array_equal(k, label[full]) and np.array_equal(E.bits(a), E.bits(aff[full]))
        for d in (4, 32):  # swapped centres (operands and norms together): the labels move
            if K > 1 + d:
                wm, cm = wc.copy(), cc.copy()
                wm[[1, 1 + d]], cm[[1, 1 + d]] = wc[[1 + d, 1]], cc[[1 + d, 1]]
                km, _ = _emulate_mfma(wm, cm, w, X[full], metric == "euclidean")
                assert not np.array_equal(km, label[full]), f"swap centres k, k + {d}"
    # the VALU kernel reads the plan's centres as they are: the same swaps on them
    plan = _plan(c, cluster_variant="valu")
    Cp, wp = plan.centers.numpy().astype(np.float64), plan.weights.numpy().astype(np.float64)
    assert np.array_equal(E.raw_distances(Cp, wp, X[ok], metric).argmin(axis=1), label[ok])
    for d in (4, 32):
        if K > 1 + d:
            Cm = Cp.copy()
            Cm[[1, 1 + d]] = Cp[[1 + d, 1]]
            assert not np.array_equal(E.raw_distances(Cm, wp, X[ok], metric).argmin(axis=1), label[ok]), d


# --------------------------------------------------------------------------- k-NN

@pytest.mark.parametrize("N,k,method,metric,F", E.KNN_CASES)
def test_knn_probe_twin_equals_oracle(N, k, method, metric, F):
    inst, targets, classes = E.knn_probe(N, k, method, metric, F)
    c = CompiledPmml.from_string(E.knn_pmml_exact(inst, targets, k, method, metric, classes))
    X = E.center_matrix(inst, 513, seed=N)
    ref, ok, tie = E.knn_reference(inst, targets, X, k, method, metric)
    so, vo = c.score_matrix_oracle(X)
    assert np.array_equal(vo, ok) and _same(so, ref)
    assert N == k or tie[ok].any()
    plan = _plan(c)
    assert isinstance(plan, KnnPlan) and plan.k == k
    s, v = _emulate_knn_kernel(plan, X.astype(np.float64))
    assert np.array_equal(v, ok) and _same(np.where(v, s, np.nan), ref)
    # instances swapped 4 and 32 apart (their targets stay): the scores move, so the rows constrain
    # which instance sits where, ties and their lower-index rule included
    inst0 = plan.inst.clone()
    for d in (4, 32) if N > k else ():  # N == k: every instance is a neighbour of every row
        pairs = [i for i in range(N - d) if targets[i] != targets[i + d] and (inst[i] != inst[i + d]).any()]
        if pairs:
            i = pairs[0]
            plan.inst = inst0.clone()
            plan.inst[[i, i + d]] = inst0[[i + d, i]]
            sm, vm = _emulate_knn_kernel(plan, X.astype(np.float64))
            assert not _same(np.where(vm, sm, np.nan), ref), f"swap instances {i}, {i + d}"
    plan.inst = inst0
