"""The matrix-core kernels (mlp.hip, gemm.hip, svm.hip, cluster.hip, knn.hip) equal the float64
oracle bit for bit on the exact-integer probes of ``tests/_exact.py``.

Every product and partial sum of a probe is an exact fp32 number (``tests/test_exact_probes.py``
proves that, and that every named mutant of the packed operands shows), so validity masks and
values are compared with ``np.array_equal`` on the bit patterns on every row: no agreement rates,
no tolerances. The two exceptions the arithmetic forces are named where they apply: the kernels
of a polynomial / RBF / sigmoid SVM are not exact (``_exact.SVM_ULP_CONSTANT``) and the affinity of a
clustering row with a missing field carries one divide, one multiply and one root (4 fp32 ulps).

Large row counts are compared with the dense float64 reference of the builder's own arrays on
every row; ``tests/test_exact_probes.py`` pins that reference to the oracle."""

import numpy as np
import pytest
import torch

import _exact as E
from flink_jpmml_amd.runtime.compiled import CompiledPmml

pytestmark = pytest.mark.gpu



def _flags_of_test_wide_mlp():
    """The ``gemm_flags`` values tests/test_wide_mlp.py sets (it compares those dispatches with one
    another; here each has to equal the oracle), read from its source so the two files cannot drift:
    ``(every value, the force values of the persistent-kernel cases)``."""
    import inspect
    import re

    import test_wide_mlp as T

    values = set()
    for line in inspect.getsource(T).splitlines():
        code = line.split("#")[0]
        if re.search(r"gemm_flags\s*=|for (flags|extra) in", code):
            values.update(int(h, 16) for h in re.findall(r"0x[0-9A-Fa-f]+", code))
    mark = [m for m in T.test_persistent_phase_kernel_matches_one_tile_per_workgroup.pytestmark
            if m.name == "parametrize"][0]
    forces = {case[2] for case in mark.args[1]}
    return sorted(values | forces), sorted(forces)


def _np(t):
    return t.cpu().numpy()


def _launch(plan, X, gpu, strided=False, **outs):
    """``plan.launch`` on ``X`` (contiguous, or as a view of a wider matrix: row stride F + 3);
    ``outs`` name extra output buffers as (shape tail, dtype). Returns (score, valid, extras)."""
    n = len(X)
    if strided:
        Xt = torch.from_numpy(E.strided(X)).to(gpu)[:, : X.shape[1]]
        assert Xt.stride(0) == X.shape[1] + 3
    else:
        Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(gpu)
    s, v = plan.alloc_outputs(n)
    extra = {k: torch.full((n,) + tuple(tail), -7, dtype=dt, device=gpu) for k, (tail, dt) in outs.items()}
    plan.launch(Xt, s, v, **extra)
    torch.cuda.synchronize()
    return _np(s).astype(np.float64), _np(v).astype(bool), {k: _np(t) for k, t in extra.items()}


def _assert_same(s, v, ref, vref, what=""):
    assert np.array_equal(v, vref), f"{what}: validity differs on rows {np.flatnonzero(v != vref)[:8]}"
    bad = np.flatnonzero(E.bits(s[v]) != E.bits(ref[v]))
    assert not len(bad), (f"{what}: {len(bad)} of {v.sum()} rows differ, first rows {np.flatnonzero(v)[bad[:5]]}: "
                          f"got {s[v][bad[:5]]}, expected {ref[v][bad[:5]]}")
    assert np.isnan(s[~v]).all()


# --------------------------------------------------------------------------- fused MLP (mlp.hip)


def _fused_kernels(plan, precision):
    if precision == "fp32":
        return ["fp32"]
    plan.set_kernel("reg")
    return ["panel", "reg"] if plan.reg_kernel else ["panel"]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(E.FUSED_SHAPES))
def test_fused_mlp_equals_oracle(gpu, name, precision):
    """Every fused-kernel variant (fp32, bf16 panel ring, bf16 register weights where the shape
    allows) on 1 / 33 / 129 / 257 rows, contiguous and strided, two models per shape; class logits
    tie on some rows (the first maximum wins) and un-normalised class outputs equal the logits."""
    from flink_jpmml_amd.runtime.nn_plans import MlpPlan

    shape = E.FUSED_SHAPES[name]
    n_all = E.nn_rows(shape["n_in"])
    for seed, norm in [(sd, nm) for sd in E.seeds(name) for nm in E.norms(shape)]:
        layers, cls, doc = E.network(shape, seed, norm)
        c = CompiledPmml.from_string(doc)
        plan = c.plan(gpu, precision=precision)
        assert type(plan) is MlpPlan
        X = E.probe_matrix(n_all, shape["n_in"], seed=seed)
        ref, vref, logits = E.nn_reference(layers, X, cls)
        so, vo = c.score_matrix_oracle(X)
        assert np.array_equal(vo, vref) and np.array_equal(E.bits(so[vo]), E.bits(ref[vo]))
        if cls:
            assert E.tie_rows(logits)[vref].any()
        for kernel in _fused_kernels(plan, precision):
            if kernel != "fp32":
                plan.set_kernel(kernel)
            for rows in sorted(set(E.ROW_COUNTS + (n_all,))):
                for strided in ((False, True) if rows == n_all else (False,)):
                    outs = dict(probs=((shape["n_out"],), torch.float32)) if cls else {}
                    s, v, ex = _launch(plan, X[:rows], gpu, strided=strided, **outs)
                    _assert_same(s, v, ref[:rows], vref[:rows],
                                 f"{name} seed {seed} {norm} {kernel} rows {rows} strided {strided}")
                    if cls and norm is None:
                        ok = vref[:rows]
                        assert np.array_equal(E.bits(ex["probs"][ok]), E.bits(logits[:rows][ok]))


@pytest.mark.parametrize("kernel", ["fp32", "panel", "reg"])
def test_fused_mlp_persistent_row_tiles(gpu, kernel):
    """70,001 rows: every persistent workgroup walks several row tiles and the last one is ragged;
    every row against the dense reference."""
    name = "64-256-256-1"
    shape = E.FUSED_SHAPES[name]
    layers, cls, doc = E.network(shape, E.seeds(name)[0])
    plan = CompiledPmml.from_string(doc).plan(gpu, precision="fp32" if kernel == "fp32" else "bf16")
    if kernel != "fp32":
        plan.set_kernel(kernel)
        assert plan.reg_kernel == (kernel == "reg")
    X = E.probe_matrix(70_001, 64, seed=7, nan_every=997)
    ref, vref, _ = E.nn_reference(layers, X, cls)
    s, v, _ = _launch(plan, X, gpu)
    _assert_same(s, v, ref, vref, kernel)


# --------------------------------------------------------------------------- wide MLP (gemm.hip)


def _wide_dispatches(plan, precision):
    """(name, attribute overrides) of every dispatch tests/test_wide_mlp.py names. The flag bits run
    with the fused head off, where every hidden layer goes through the flagged launch, as they do
    there; the bits that file also sets with the fused head on (none but the force bits: 0x40,
    0x1000) run that way too. A fused-input case is kept only where the first layer really takes
    the fused input stage."""
    out = [("default", {})]
    if precision == "bf16":
        out.append(("fuse_head off", dict(fuse_head=False)))
        for over in (dict(fuse_input=True), dict(fuse_input=True, fuse_head=False)):
            if _with(plan, over, lambda: plan._fused_input(plan._fused_head())):
                out.append((", ".join(f"{k} {v}" for k, v in over.items()), over))
        flags, forces = _flags_of_test_wide_mlp()
        for f in flags:
            if f:
                out.append((f"flags {f:#x}, fuse_head off", dict(gemm_flags=f, fuse_head=False)))
                if f in (0x40, 0x1000):
                    out.append((f"flags {f:#x}", dict(gemm_flags=f)))
    if plan.in_contig:
        out.append(("in_contig 0", dict(in_contig=0)))
    return out


def _with(plan, over, fn):
    saved = {k: getattr(plan, k) for k in over}
    try:
        for k, val in over.items():
            setattr(plan, k, val)
        return fn()
    finally:
        for k, val in saved.items():
            setattr(plan, k, val)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(E.WIDE_SHAPES))
def test_wide_mlp_every_dispatch_equals_oracle(gpu, name, precision):
    """Every dispatch of the wide GEMM (default, fused head off, fused input stage, per-input
    gather, each experiment bit) equals the oracle itself, not another variant, on 1 / 33 / 129 /
    257 rows and on a batch that holds every one-hot row; the shapes cover the K = 64 first-layer
    kernels, K >= 512, the input stage above 1024 inputs, 32-unit output groups with the wide decode
    and the 4-class fused head. Un-normalised ``probs=`` equal the integer logits."""
    from flink_jpmml_amd.runtime.nn_plans import WideMlpPlan

    shape = E.WIDE_SHAPES[name]
    n_in = shape["n_in"]
    rows_all = E.nn_rows(n_in)  # every one-hot row is in
    for seed, norm in [(sd, nm) for sd in E.seeds(name) for nm in E.norms(shape)]:
        layers, cls, doc = E.network(shape, seed, norm)
        c = CompiledPmml.from_string(doc)
        plan = c.plan(gpu, precision=precision)
        assert type(plan) is WideMlpPlan and plan.bf16 == (precision == "bf16")
        X = E.probe_matrix(rows_all, n_in, seed=seed)
        ref, vref, logits = E.nn_reference(layers, X, cls)
        idx = np.arange(0, rows_all, 1 if n_in * shape["hidden"][0] < 40_000 else 9)
        so, vo = c.score_matrix_oracle(X[idx])  # the per-connection oracle: a fixed subsample of the big nets
        assert np.array_equal(vo, vref[idx]) and np.array_equal(E.bits(so[vo]), E.bits(ref[idx][vo]))
        if cls:
            assert E.tie_rows(logits)[vref].any()
        outs = dict(probs=((shape["n_out"],), torch.float32)) if cls else {}
        for dname, over in _wide_dispatches(plan, precision):
            for rows in sorted(set(E.ROW_COUNTS + (rows_all,))):
                views = (False, True) if rows == rows_all and (dname == "default" or "fuse_input" in over) else (False,)
                for strided in views:
                    def run():
                        assert plan._fused_input(plan._fused_head()) == bool(over.get("fuse_input"))
                        return _launch(plan, X[:rows], gpu, strided=strided, **outs)

                    s, v, ex = _with(plan, over, run)
                    _assert_same(s, v, ref[:rows], vref[:rows],
                                 f"{name} seed {seed} {norm} {dname} rows {rows} strided {strided}")
                    if cls and norm is None:
                        ok = vref[:rows]
                        assert np.array_equal(E.bits(ex["probs"][ok]), E.bits(logits[:rows][ok])), dname


@pytest.mark.parametrize("name", ["65-257-300-1", "64-512-1", "40-300-1024-1", "24-512-768-4cls"])
def test_wide_mlp_persistent_tile_walk_equals_reference(gpu, name):
    """41,000 rows (322 row tiles of the persistent K = 64 kernel, a ragged last one; more tiles
    than workgroups on the phase-interleaved layers): the default persistent kernels, one tile per
    workgroup (bit 12) and the forced phase kernels, fused head on and off, every row against the
    dense reference."""
    shape = E.WIDE_SHAPES[name]
    layers, cls, doc = E.network(shape, E.seeds(name)[0])
    plan = CompiledPmml.from_string(doc).plan(gpu, precision="bf16")
    X = E.probe_matrix(41_000, shape["n_in"], seed=11, nan_every=997)
    ref, vref, _ = E.nn_reference(layers, X, cls)
    forces = _flags_of_test_wide_mlp()[1]
    assert 0x80 in forces and 0xC0 in forces and 0 in forces
    for fuse in (True, False):
        for force in forces:
            for extra in (0, 0x1000):
                if fuse and force:
                    continue  # the forced kernels are hidden-layer launches
                over = dict(fuse_head=fuse, gemm_flags=force | extra)
                s, v, _ = _with(plan, over, lambda: _launch(plan, X, gpu))
                _assert_same(s, v, ref, vref, f"{name} fuse_head {fuse} flags {force | extra:#x}")


# --------------------------------------------------------------------------- SVM (svm.hip)


@pytest.mark.parametrize("name", list(E.SVM_CASES))
def test_linear_svm_decisions_and_labels_equal_oracle(gpu, name):
    """Linear kernel, integer data: the whole [rows, machines] ``decision=`` array equals
    ``decision_values`` bit for bit and the labels equal the oracle's on every row, with at least
    1 % of the rows holding a decision value exactly on the threshold."""
    p, kind = E.svm_probe(name)
    c = CompiledPmml.from_string(p.pmml())
    plan = c.plan(gpu)
    assert type(plan).__name__ == kind
    X = E.svm_matrix(E.SVM_ROWS, p.F)
    ref, vref, D = p.reference(X)
    so, vo = c.score_matrix_oracle(X)
    assert np.array_equal(vo, vref) and np.array_equal(E.bits(so[vo]), E.bits(ref[vo]))
    assert np.array_equal(c.evaluator.decision_values(np.nan_to_num(X.astype(np.float64))), D)
    if p.n_classes >= 2:
        assert ((D == 0).any(axis=1) & vref).mean() >= 0.01
    M = D.shape[1]
    for rows in E.ROW_COUNTS + (E.SVM_ROWS,):
        for strided in ((False, True) if rows == 257 else (False,)):
            s, v, ex = _launch(plan, X[:rows], gpu, strided=strided, decision=((M,), torch.float32))
            what = f"{name} rows {rows} strided {strided}"
            _assert_same(s, v, ref[:rows], vref[:rows], what)
            ok = vref[:rows]
            assert np.array_equal(E.bits(ex["decision"][ok]), E.bits(D[:rows][ok])), what


@pytest.mark.parametrize("kernel", ["polynomial", "radialBasis", "sigmoid"])
@pytest.mark.parametrize("name", E.NONLINEAR_SVM_CASES)
def test_nonlinear_svm_decisions_within_scaled_bound(gpu, name, kernel):
    """Polynomial, RBF and sigmoid kernels are not exact: every ``decision=`` entry is within
    ``_exact.SVM_ULP_CONSTANT * 2^-24 * (sum_j |a_jm| |K_j| (1 + |arg_j|) + |D|)`` of the float64 oracle.
    Largest ratio measured on the MI355X over these cases: 1.648 (wide kernel, 12 classes, RBF);
    the constant is 4 x 1.65 = 6.6."""
    p, kind = E.svm_probe(name, kernel=kernel)
    c = CompiledPmml.from_string(p.pmml())
    plan = c.plan(gpu)
    assert type(plan).__name__ == kind
    X = E.svm_matrix(513, p.F, seed=6)
    ok = ~np.isnan(X).any(axis=1)
    D, T = p.kernel_terms(X)
    Do = c.evaluator.decision_values(np.nan_to_num(X.astype(np.float64)))
    np.testing.assert_allclose(Do, D, rtol=1e-12, atol=1e-12)
    s, v, ex = _launch(plan, X, gpu, decision=((D.shape[1],), torch.float32))
    assert np.array_equal(v, ok)
    ratio = np.abs(ex["decision"][ok].astype(np.float64) - Do[ok]) / (2.0 ** -24 * T[ok])
    print(f"svm ratio {name} {kernel}: {ratio.max():.4f}")
    assert ratio.max() <= E.SVM_ULP_CONSTANT


# --------------------------------------------------------------------------- clustering (cluster.hip)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("variant,metric", [("valu", "squaredEuclidean"), ("valu", "euclidean"), ("valu", "cityBlock"),
                                            ("valu", "chebychev"), ("mfma", "squaredEuclidean"), ("mfma", "euclidean")])
@pytest.mark.parametrize("K,F", E.CLUSTER_CASES)
def test_cluster_labels_and_affinity_equal_oracle(gpu, K, F, metric, variant):
    """Duplicate centres 4 apart (the other lane half) and 32 apart (the next tile) and distinct
    equidistant centres: the first minimum wins on every row, rows with a missing field included;
    ``affinity=`` is bit-equal on complete rows (euclidean: the correctly rounded fp32 root of the
    exact sum) and within 4 fp32 ulps where a field is missing (one divide, one multiply, one root)."""
    from flink_jpmml_amd.runtime.plans import compile_plan

    C, w = E.grid_centers(K, F, seed=K), E.field_weights(F, seed=F)
    c = CompiledPmml.from_string(E.cluster_pmml(C, w, metric))
    plan = compile_plan(c, gpu, cluster_variant=variant)
    assert plan.variant == variant
    X = E.center_matrix(C, 513, seed=K + F)
    label, aff, vref, raw = E.cluster_reference(C, w, X, metric)
    so, vo = c.score_matrix_oracle(X)
    assert np.array_equal(vo, vref) and np.array_equal(so[vo], label[vo] + 1.0)
    oracle_aff = c.result(X).affinity
    full = ~np.isnan(X).any(axis=1)
    assert np.array_equal(oracle_aff[full], aff[full])
    assert E.min_tie_rows(raw)[vref].any() and (F == 1 or (vref & ~full).any())
    ref = np.where(vref, label + 1.0, np.nan)
    for rows in E.ROW_COUNTS + (len(X),):
        for strided in ((False, True) if rows == 257 else (False,)):
            s, v, ex = _launch(plan, X[:rows], gpu, strided=strided, label=((), torch.int32),
                               affinity=((), torch.float32))
            what = f"rows {rows} strided {strided}"
            _assert_same(s, v, ref[:rows], vref[:rows], what)
            ok, fl = vref[:rows], full[:rows]
            assert np.array_equal(ex["label"][ok], label[:rows][ok]), what
            assert np.array_equal(E.bits(ex["affinity"][fl]), E.bits(aff[:rows][fl].astype(np.float32))), what
            part = ok & ~fl
            assert (_ulps(ex["affinity"][part], oracle_aff[:rows][part].astype(np.float32)) <= 4).all(), what


# --------------------------------------------------------------------------- k-NN (knn.hip)


@pytest.mark.parametrize("variant", ["valu", "mfma"])
@pytest.mark.parametrize("N,k,method,metric,F", E.KNN_CASES)
def test_knn_scores_equal_oracle(gpu, N, k, method, metric, F, variant):
    """Instances on an integer grid with duplicates 4 and 32 apart: rows whose k-th and (k+1)-th
    neighbours are equidistant exist and the lower index wins; votes, odd-k medians and power-of-two
    averages of integer targets are exact, so scores and validity are equal on every row."""
    from flink_jpmml_amd.runtime.plans import KnnPlan
    inst, targets, classes = E.knn_probe(N, k, method, metric, F)
    c = CompiledPmml.from_string(E.knn_pmml_exact(inst, targets, k, method, metric, classes))
    plan = c.plan(gpu, knn_variant=variant)
    assert isinstance(plan, KnnPlan) and plan.variant == variant and plan.k == k
    X = E.center_matrix(inst, 513, seed=N)
    ref, vref, tie = E.knn_reference(inst, targets, X, k, method, metric)
    so, vo = c.score_matrix_oracle(X)
    assert np.array_equal(vo, vref) and np.array_equal(E.bits(so[vo]), E.bits(ref[vo]))
    assert N == k or tie[vref].any()
    for rows in E.ROW_COUNTS + (len(X),):
        for strided in ((False, True) if rows == 257 else (False,)):
            s, v, _ = _launch(plan, X[:rows], gpu, strided=strided)
            _assert_same(s, v, ref[:rows], vref[:rows], f"rows {rows} strided {strided}")
