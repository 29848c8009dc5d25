"""Every activation at every site of the network kernels (mlp.hip, gemm.hip), and the four copies
of the softmax / simplemax row normalisation, against the float64 reference of
``tests/_act_cases.py`` on the device.

The pre-activations are exact (``tests/test_act_cases.py`` proves it, and that the oracle equals
the reference and every named mutant shows), so identity, rectifier, square, threshold, reciprocal
and Elliott are compared bit for bit and the seven smooth functions within
``C_f 2^-24 S_f(z)``, with the constants measured on the MI355X (``_act_cases.MEASURED_RATIO``).
Every valid row is compared and validity is compared exactly: no agreement rates."""

import numpy as np
import pytest
import torch

import _act_cases as A
import _exact as E
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.nn_plans import MlpPlan, WideMlpPlan
from test_gpu_exact import _fused_kernels, _launch, _wide_dispatches, _with

pytestmark = pytest.mark.gpu

FP32_MAX = float(np.finfo(np.float32).max)


def _dispatches(plan, precision, fused):
    """``[(label, overrides, set_kernel name or None)]``: fp32 / bf16 panel / bf16 register kernel of
    the fused plan; the default dispatch and the fused head off of the wide plan."""
    if fused:
        return [(k, {}, None if k == "fp32" else k) for k in _fused_kernels(plan, precision)]
    return [(n, over, None) for n, over in _wide_dispatches(plan, precision) if n in ("default", "fuse_head off")]


def _hidden_rounded(precision, label, r) -> bool:
    """Does this kernel carry the tested hidden layer's activation as bf16? Every bf16 kernel does,
    but the register kernel with the folded output layer (at most 4 outputs): it dots the last hidden
    layer's fp32 accumulators with the output weights, so that layer's activation is never rounded."""
    hidden = r.tested < len(r.sizes) - 1
    folded = label == "reg" and r.n_out <= 4 and r.tested == len(r.sizes) - 2
    return precision == "bf16" and hidden and not folded


def _run(plan, kernel, over, X, gpu, n_out, strided=False):
    if kernel is not None:
        plan.set_kernel(kernel)
        assert plan.reg_kernel == (kernel == "reg")
    outs = dict(probs=((n_out,), torch.float32)) if n_out > 1 else {}
    s, v, ex = _with(plan, over, lambda: _launch(plan, X, gpu, strided=strided, **outs))
    return s, v, (ex["probs"] if n_out > 1 else s.astype(np.float32)[:, None])


def _batches(seed):
    """(rows, strided) of one seed: 1 / 33 / 129 / 257 rows and the strided view once."""
    return [(n, False) for n in E.ROW_COUNTS] + [(A.ROWS, True)] if seed == 0 else [(A.ROWS, False)]


def _compare(r, got, s, v, want, tol, ref, valid, z, bf16_hidden, what, ratios, key):
    """One launch against the rule of its case; the largest ratio of a bounded function is kept."""
    with np.errstate(invalid="ignore"):
        vwant = valid if r.classification else valid & (np.abs(want[:, 0]) <= FP32_MAX)
    assert np.array_equal(v, vwant), f"{what}: validity differs on rows {np.flatnonzero(v != vwant)[:8]}"
    assert np.isnan(s[~v]).all(), what
    g = got[v]
    if tol is None:
        bad = np.argwhere(E.bits(g) != E.bits(want[v]))
        assert not len(bad), f"{what}: {len(bad)} entries differ, first {bad[:4].tolist()}: got " \
                             f"{g[tuple(bad[0])]!r}, expected {want[v][tuple(bad[0])]!r} at z = {z[v][tuple(bad[0])]}"
        label = want[v].argmax(axis=1)
    else:
        d = np.abs(g.astype(np.float64) - ref[v])
        slack = A.half_bf16_ulp(ref[v]) if bf16_hidden else 0.0
        ratio = float((np.maximum(d - slack, 0.0) / (A.U * A.scale(r.act, z[v], ref[v]))).max()) if len(d) else 0.0
        ratios[key] = max(ratios.get(key, 0.0), ratio)
        worst = np.unravel_index(np.argmax(d - tol[v]), d.shape) if len(d) else None
        assert (d <= tol[v]).all(), f"{what}: ratio {ratio:.3f} > C = {A.C[r.act]}, worst at z = {z[v][worst]}: " \
                                    f"got {g[worst]!r}, reference {ref[v][worst]!r}"
        if bf16_hidden:
            assert A.is_bf16(g).all(), f"{what}: a hidden activation of a bf16 kernel is no bf16 number"
        label = g.argmax(axis=1)
    if r.classification:  # the first maximum of the class outputs
        assert np.array_equal(s[v], label.astype(np.float64)), what


@pytest.mark.parametrize("name,tested", A.SITES)
def test_activation_at_site_equals_reference(gpu, name, tested):
    """All 13 activations (threshold 0.25 set on the layer, then on the network) at one site of one
    kernel path: fp32, bf16 panel and bf16 register kernels of the fused plan, default dispatch and
    fused head off of the wide plan; 1 / 33 / 129 / 257 rows, a strided view, NaN cells; two models."""
    fused = name in A.FUSED_PATHS
    out_site = A.is_output_site(name, tested)
    n_out = A.PATHS[name][2]
    ratios = {}
    for variant in A.VARIANTS:
        for seed in A.SEEDS:
            r = A.ramp(name, tested, variant, seed)
            X = A.ramp_matrix(A.ROWS, r.n_in, seed)
            c = CompiledPmml.from_string(r.pmml())
            for precision in ("fp32", "bf16"):
                plan = c.plan(gpu, precision=precision)
                assert type(plan) is (MlpPlan if fused else WideMlpPlan)
                disp = _dispatches(plan, precision, fused)
                if precision == "bf16":
                    if name.startswith("64-256-256"):
                        assert [d[0] for d in disp] == ["panel", "reg"]
                    if not fused:
                        assert [d[0] for d in disp] == ["default", "fuse_head off"]
                        assert plan._fused_head() == (len(r.sizes) >= 2 and n_out <= 32)
                for label, over, kernel in disp:
                    bf16_hidden = _hidden_rounded(precision, label, r)
                    want, tol, ref, valid, z = A.expected(r, X, bf16_hidden)
                    for rows, strided in _batches(seed):
                        s, v, got = _run(plan, kernel, over, X[:rows], gpu, n_out, strided)
                        _compare(r, got, s, v, want[:rows], None if tol is None else tol[:rows], ref[:rows],
                                 valid[:rows], z[:rows], bf16_hidden,
                                 f"{name} layer {tested} {variant[0]} seed {seed} {precision} {label} rows {rows} "
                                 f"strided {strided}", ratios, (r.act, f"{precision} {label}"))
    for (act, where), ratio in sorted(ratios.items()):
        print(f"ACT_RATIO {act} | {name} layer {tested}{' (output)' if out_site else ''} | {where} | {ratio:.4f}")


@pytest.mark.parametrize("name", A.TWO_SITE)
def test_two_sites_keep_their_own_activation(gpu, name):
    """Rectifier in the hidden layer, square in the output layer, bit for bit: neither site takes
    the other's code."""
    fused = name in A.FUSED_PATHS
    for seed in A.SEEDS:
        r = A.ramp(name, 0, ("rectifier", "rectifier", None, None), seed, post_act="square")
        X = A.ramp_matrix(A.ROWS, r.n_in, seed)
        c = CompiledPmml.from_string(r.pmml())
        for precision in ("fp32", "bf16"):
            plan = c.plan(gpu, precision=precision)
            for label, over, kernel in _dispatches(plan, precision, fused):
                want, tol, ref, valid, z = A.expected(r, X, False)
                assert tol is None
                if _hidden_rounded(precision, label, r):  # the rectified z is rounded to bf16 before the square
                    want = A.twin_activate("square", A.bf16_rn(np.maximum(z, 0.0).astype(np.float32)))
                s, v, got = _run(plan, kernel, over, X, gpu, 1)
                _compare(r, got, s, v, want, None, ref, valid, z, False, f"{name} seed {seed} {precision} {label}",
                         {}, None)


# --------------------------------------------------------------------------- row normalisation


@pytest.mark.parametrize("name", list(A.NORM_FUSED) + list(A.NORM_WIDE))
def test_row_normalisation_equals_reference(gpu, name):
    """softmax, simplemax and no normalisation over small exact logits at one output width, on every
    kernel that decodes it. simplemax: probabilities bit-equal to fp32(z_u / sum z), labels the
    oracle's, rows with a negative and a power-of-two sum included; rows whose logits sum to 0 are
    invalid with a NaN score. softmax: within SOFTMAX_C 2^-24 (p (1 + mx - z_u) + (n_out - 1) p) of the
    float64 reference, duplicated logits bit-equal, the first maximum wins, rows sum to 1 within n_out
    ulps. None: the logits themselves."""
    fused = name in A.NORM_FUSED
    n_in, hidden, n_out = (A.NORM_FUSED if fused else A.NORM_WIDE)[name]
    net = A.Logits(n_in, hidden, n_out)
    X = net.matrix(A.ROWS)
    Z, valid = net.logits(X)
    sums = Z.sum(axis=1)
    worst = 0.0
    for norm in A.NORMS:
        c = CompiledPmml.from_string(net.pmml(norm))
        P, label, S = A.norm_reference(Z, norm)
        zero = valid & (sums == 0) if norm == "simplemax" else np.zeros(len(X), bool)
        ok = valid & ~zero
        for precision in ("fp32", "bf16"):
            plan = c.plan(gpu, precision=precision)
            assert type(plan) is (MlpPlan if fused else WideMlpPlan)
            disp = _dispatches(plan, precision, fused)
            if precision == "bf16" and name.startswith("64-256-256"):
                assert [d[0] for d in disp] == ["panel", "reg"]
            for dlabel, over, kernel in disp:
                for rows, strided in _batches(0):
                    s, v, p = _run(plan, kernel, over, X[:rows], gpu, n_out, strided)
                    what = f"{name} {norm} {precision} {dlabel} rows {rows} strided {strided}"
                    o = ok[:rows]
                    assert np.array_equal(v, o), f"{what}: validity differs on rows {np.flatnonzero(v != o)[:8]}"
                    assert np.isnan(s[~v]).all(), what
                    assert np.array_equal(s[o], label[:rows][o].astype(np.float64)), what
                    if norm == "softmax":
                        d = np.abs(p[o].astype(np.float64) - P[:rows][o])
                        ratio = float((d / (A.U * S[:rows][o])).max())
                        worst = max(worst, ratio)
                        assert ratio <= A.SOFTMAX_C, f"{what}: ratio {ratio:.3f}"
                        assert (np.abs(p[o].astype(np.float64).sum(axis=1) - 1.0) <= n_out * 2.0 ** -23).all(), what
                        if n_out >= 4:
                            assert np.array_equal(E.bits(p[o][:, -1]), E.bits(p[o][:, net.dup])), what
                    else:
                        assert np.array_equal(E.bits(p[o]), E.bits(P[:rows][o].astype(np.float32))), what
    print(f"SOFTMAX_RATIO {name} | {worst:.4f}")


# --------------------------------------------------------------------------- poles and overflow

# (a, b) of the units no output reads: off every pole; the table is longer than any layer here, so
# only the read unit takes its first entry
OFF_POLE = [(1, 1 / 32), (-1, 1 / 32), (2, 1 / 32), (-2, 1 / 32)] * 100
EDGE_PATHS = {"17-1-1": (17, (1,), 1), "17-33-1": (17, (33,), 1), "33-300-1": (33, (300,), 1)}


def _edge_launches(r, gpu):
    X = A.ramp_matrix(A.ROWS, r.n_in, 0)
    c = CompiledPmml.from_string(r.pmml())
    so, vo = c.score_matrix_oracle(X)
    fused = r.sizes[0] <= 256
    for precision in ("fp32", "bf16"):
        plan = c.plan(gpu, precision=precision)
        assert type(plan) is (MlpPlan if fused else WideMlpPlan)
        for label, over, kernel in _dispatches(plan, precision, fused):
            s, v, _ = _run(plan, kernel, over, X, gpu, 1)
            yield f"{precision} {label}", _hidden_rounded(precision, label, r), X, s, v, so, vo


@pytest.mark.parametrize("name", list(EDGE_PATHS))
def test_pole_on_a_read_unit_invalidates_the_row(gpu, name):
    """reciprocal at z = 0 on the unit the output reads (every other unit is off the pole; the
    one-unit layer has only padded neighbours): the row is invalid with a NaN score, as in the
    oracle; every other row is bit-equal."""
    n_in, hidden, n_out = EDGE_PATHS[name]
    r = A.Ramp(n_in, hidden, n_out, 0, "reciprocal", 0, pole_shift=0.0, ab=[(4, 0.0)] + OFF_POLE)
    ref, valid, z = r.reference(A.ramp_matrix(A.ROWS, n_in, 0))
    assert (z[valid] == 0).any()
    for what, rounded, X, s, v, so, vo in _edge_launches(r, gpu):
        assert r.unread_poles(X) == 0
        assert np.array_equal(vo, valid & (z[:, 0] != 0)) and np.array_equal(v, vo), what
        assert np.isnan(s[~v]).all(), what
        want = ref[:, 0].astype(np.float32)
        if rounded:
            want = A.bf16_rn(want)
        assert np.array_equal(E.bits(s[v]), E.bits(want[v])), what


@pytest.mark.parametrize("name", list(EDGE_PATHS))
def test_exponential_past_fp32_range_is_invalid_on_the_device(gpu, name):
    """exponential of z in 64 .. 96 on the read unit: from z = 88.75 on, exp(z) exceeds fp32's range.
    The float64 oracle still scores those rows (a deliberate deviation, docs/PARITY.md); the device
    row is invalid with a NaN score. Below, the bound of the exponential holds."""
    n_in, hidden, n_out = EDGE_PATHS[name]
    r = A.Ramp(n_in, hidden, n_out, 0, "exponential", 0, ab=[(4, 80.0)] + OFF_POLE)
    ref, valid, z = r.reference(A.ramp_matrix(A.ROWS, n_in, 0))
    over = ref[:, 0] > FP32_MAX
    assert (over & valid).any() and np.isfinite(ref).all() and z[over].min() == 88.75 and z[~over].max() == 88.5
    for what, rounded, X, s, v, so, vo in _edge_launches(r, gpu):
        assert r.unread_poles(X) == 0
        assert np.array_equal(vo, valid) and np.array_equal(so[valid], ref[valid, 0]), what
        assert np.array_equal(v, valid & ~over), what
        assert np.isnan(s[~v]).all(), what
        tol = A.bound("exponential", z[:, 0], ref[:, 0], rounded)
        assert (np.abs(s[v] - ref[v, 0]) <= tol[v]).all(), what


@pytest.mark.parametrize("name", ["17-33-1", "33-300-1"])
def test_pole_on_an_unread_unit_invalidates_the_row_on_the_device(gpu, name):
    """reciprocal at z = 0 on a hidden unit that the output does not read (no stored connection). The
    oracle sums stored connections only and scores the row; the dense kernels multiply the unit's inf
    by the stored zero and the row is invalid with a NaN score (a deliberate deviation,
    docs/PARITY.md). Pinned: the device row is valid exactly where no unit of the layer sits on the
    pole, and bit-equal there."""
    n_in, hidden, n_out = EDGE_PATHS[name]
    r = A.Ramp(n_in, hidden, n_out, 0, "reciprocal", 0, pole_shift=0.0)
    X = A.ramp_matrix(A.ROWS, n_in, 0)
    ref, valid, z = r.reference(X)
    any_pole = (r.z_all(X) == 0).any(axis=1)
    assert r.unread_poles(X) > 0 and (valid & any_pole & (z[:, 0] != 0)).any() and (valid & ~any_pole).any()
    for what, rounded, X, s, v, so, vo in _edge_launches(r, gpu):
        assert np.array_equal(vo, valid & (z[:, 0] != 0)), what
        assert np.array_equal(v, valid & ~any_pole), what
        assert np.isnan(s[~v]).all(), what
        want = ref[:, 0].astype(np.float32)
        if rounded:
            want = A.bf16_rn(want)
        assert np.array_equal(E.bits(s[v]), E.bits(want[v])), what


def test_library_gemm_plan_gives_zero_sum_simplemax_rows_no_prediction(gpu):
    """The library-GEMM plan (``mlp_impl="gemm"``) follows the kernels' rule: a simplemax row whose
    logits sum to 0 has no prediction; every other row keeps the oracle's validity and label."""
    from flink_jpmml_amd.runtime.nn_plans import GemmMlpPlan

    net = A.Logits(12, (40,), 7)
    X = net.matrix(A.ROWS)
    Z, valid = net.logits(X)
    P, label, _ = A.norm_reference(Z, "simplemax")
    ok = valid & (Z.sum(axis=1) != 0)
    assert (valid & ~ok).any()
    plan = CompiledPmml.from_string(net.pmml("simplemax")).plan(gpu, precision="fp32", mlp_impl="gemm")
    assert type(plan) is GemmMlpPlan
    s, v, ex = _launch(plan, X, gpu, probs=((7,), torch.float32))
    assert np.array_equal(v, ok) and np.isnan(s[~v]).all()
    single = ok.copy()
    single[ok] = ~E.tie_rows(P[ok])  # this plan's arg-max is the library's: compared where the maximum is single
    assert np.array_equal(s[single], label[single].astype(np.float64))
    np.testing.assert_allclose(ex["probs"][ok], P[ok], rtol=1e-6, atol=0)
