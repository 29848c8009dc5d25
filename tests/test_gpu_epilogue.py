"""The score epilogue (csrc/epilogue.h, common.h::apply_link) and linear.hip on exact-eta probes
(GPU side of tests/_epilogue_cases.py; tests/test_epilogue_cases.py proves the grids on the CPU).

Every eta is an exact fp32 number in any summation order, so the kernel starts from the bits of
the float64 reference: validity, labels and every score the arithmetic makes exact (numeric class
labels, link ``none``, cast Target values, simplemax over a power-of-two sum) are compared with
``np.array_equal`` on every row; probabilities and link values against ``C 2^-24`` with the
per-link constants of ``_epilogue_cases.C_BOUND``. The only rows on which the device may differ from
the oracle are those of the fp32 model-value rule (docs/PARITY.md, "Deliberate deviations"), which
the reference takes as a flag. No agreement rates, no row left out."""

import functools

import numpy as np
import pytest
import torch

from tests import _boundary as B
from tests import _epilogue_cases as E
from tests import _exact as X_

from flink_jpmml_amd.bench.synth import gbdt_pmml, set_target
from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import lowering_dry_run

pytestmark = pytest.mark.gpu

F32 = np.float32
ROW_COUNTS = (1, 255, 256, 257)  # one ragged 256-row tile, one 1-row tile
LAYOUTS = ("contiguous", "odd-stride", "stride4")
RATIOS = {}  # norm -> (largest |device - reference| / (2^-24 magnitude) seen in this session, where)


# --------------------------------------------------------------------------- linear kernel

# (K, F, norms, sparse); every (mode, link) pair that lowers appears at K = 0 / 2 / 3
ALL = E.CLASS_NORMS
LINEAR = [(1, 1, ("softmax", "logit"), False), (1, 5, ALL, False), (2, 1, ALL, False), (2, 5, ALL, False), (2, 63, ("softmax", "logit"), False), (2, 128, ("logit", "none"), False),
          (3, 5, ("softmax", "logit", "cauchit"), False), (3, 63, ALL, False), (3, 64, ("softmax", "simplemax", "probit"), False),
          (16, 63, ("softmax", "logit"), False), (16, 64, ("softmax", "simplemax", "logit", "none"), False),
          (16, 128, ("softmax", "loglog"), False),
          (2, 2, ALL, True), (3, 3, ALL, True), (16, 16, ("softmax", "simplemax", "none", "logit"), True)]
LINEAR_IDS = [(K, F, norm, sp) for K, F, norms, sp in LINEAR for norm in norms]


@functools.lru_cache(maxsize=None)
def linear_case(K, F, norm, sparse=False, zero=None, target=None):
    case = E.classification_case(K, F, norm, sparse, zero) if K else E.regression_case(F, norm, target)
    return case, CompiledPmml.from_string(case.probe.pmml()), case.reference(fp32_rule=True)


def _view(X: np.ndarray, layout: str, device):
    """The input on the device: contiguous; a column view of a wider matrix whose row stride is not
    a multiple of 4 (the scalar staging path of ``stage_rows_T``); or one whose stride is a
    multiple of 4 (the float4 path, whose last quad then reads past F into the padding)."""
    n, F = X.shape
    if layout == "contiguous":
        return torch.from_numpy(np.ascontiguousarray(X)).to(device)
    ld = F + 3 if (F + 3) % 4 else F + 1
    if layout == "stride4":
        ld = (F + 4) // 4 * 4 + (4 if F % 4 == 0 else 0)
    wide = np.full((n, ld), 97.0, dtype=F32)
    wide[:, :F] = X
    t = torch.from_numpy(wide).to(device)[:, :F]
    assert t.stride(0) == ld and (ld % 4 == 0) == (layout == "stride4")
    return t


def _launch(plan, Xt, C):
    n = Xt.shape[0]
    dev = Xt.device
    s, v = plan.alloc_outputs(n)
    s2, v2 = plan.alloc_outputs(n)
    probs = torch.full((n, C), -7.0, dtype=torch.float32, device=dev)
    kw = dict(score2=s2, valid2=v2) if type(plan).__name__ == "LinearPlan" else {}
    plan.launch(Xt, s, v, probs=probs, **kw)
    torch.cuda.synchronize()
    s, v = s.cpu().numpy(), v.cpu().numpy().astype(bool)
    if kw:  # the mirrors carry the same bits
        assert np.array_equal(X_.bits(s2.cpu().numpy()), X_.bits(s)) and np.array_equal(v2.cpu().numpy().astype(bool), v)
    return s, v, probs.cpu().numpy()


def _ratio(norm, got, ref, mag=None, what=""):
    if not ref.size:
        return 0.0
    q = np.abs(got.astype(np.float64) - ref) / E.value_bound(norm, ref if mag is None else mag, 1.0)
    i = np.unravel_index(int(q.argmax()), q.shape)
    r = float(q[i])
    if r > RATIOS.get(norm, (0.0, ""))[0]:
        RATIOS[norm] = (r, f"{what} at {i}: device {got[i]!r}, reference {ref[i]!r}")
    return r


def _check(what, s, v, probs, ref, K, norm, rows=slice(None), exact_values=False):
    """Device outputs of ``rows`` against the reference (computed once for the whole grid)."""
    rv, rs, rp, fl = ref["valid"][rows], ref["score"][rows], ref["probs"][rows], ref["flagged"][rows]
    assert np.array_equal(v, rv), f"{what}: validity differs on rows {np.flatnonzero(v != rv)[:8]}"
    assert np.isnan(s[~rv]).all()
    link = norm.split(":")[-1]
    if K or exact_values:
        bad = np.flatnonzero(s[rv] != rs[rv].astype(F32))
        assert not len(bad), f"{what}: {len(bad)} scores differ, first rows {np.flatnonzero(rv)[bad][:8]}"
    if not K and exact_values:
        return 0.0
    ok = rv & ~fl & np.isfinite(rp).all(axis=1)
    got = probs[ok] if K else s[ok, None]
    want = rp[ok]
    if link == "none" and norm != "simplemax":
        assert np.array_equal(X_.bits(got), X_.bits(want.astype(F32))), f"{what}: link none is exact"
        return 0.0
    if norm == "simplemax" and len(want) > 64:
        # a power-of-two sum divides exactly: every quotient that is an fp32 number compares bit for bit
        pow2 = (want.astype(F32).astype(np.float64) == want).all(axis=1)
        assert pow2.sum() >= 8
        assert np.array_equal(X_.bits(got[pow2]), X_.bits(want[pow2].astype(F32))), f"{what}: exact simplemax rows"
    key = norm if norm in ("softmax", "simplemax") else link
    r = _ratio(key, got, want, E.magnitudes(K, norm, want) if K else None, what)
    assert r <= E.C_BOUND[key], f"{what}: |device - reference| = {r:.3f} x 2^-24, bound {E.C_BOUND[key]}"
    return r


@pytest.mark.parametrize("K,F,norm,sparse", LINEAR_IDS, ids=[f"K{k}-F{f}-{n}{'-sparse' if s else ''}" for k, f, n, s in LINEAR_IDS])
def test_linear_classification(gpu, K, F, norm, sparse):
    """Every classification epilogue of linear.hip: softmax, simplemax, the two-table rule and the
    per-class links, dense and sparse tables, three input layouts, four row counts."""
    case, c, ref = linear_case(K, F, norm, sparse)
    plan = PL.LinearPlan(c, gpu)
    assert plan.epi_args["mode"] == E.epilogue_mode(K, norm) and (plan.listed is not None) == sparse
    worst = 0.0
    for layout in LAYOUTS:
        s, v, probs = _launch(plan, _view(case.X, layout, gpu), K)
        worst = max(worst, _check(f"{case.name} {layout}", s, v, probs, ref, K, norm))
    for n in ROW_COUNTS:
        s, v, probs = _launch(plan, _view(case.X[:n], "contiguous", gpu), K)
        _check(f"{case.name} {n} rows", s, v, probs, ref, K, norm, slice(0, n))
    print(f"{case.name}: {len(case.X)} rows, largest ratio {worst:.3f} x 2^-24")


def test_explicit_zero_coefficient_still_meets_infinity(gpu):
    """A predictor a table does not list is not multiplied (an infinite input leaves that table's
    eta alone, as in the oracle); an explicit ``coefficient="0"`` is, and 0 * inf voids the row."""
    case, c, ref = linear_case(3, 3, "logit", True, (1, 0))
    plan = PL.LinearPlan(c, gpu)
    s, v, probs = _launch(plan, _view(case.X, "contiguous", gpu), 3)
    _check(case.name, s, v, probs, ref, 3, "logit")
    inf_rows = np.isinf(case.X[:, 1])
    assert inf_rows.any() and not ref["valid"][inf_rows].any()
    plain, _, pref = linear_case(3, 3, "logit", True)
    assert pref["valid"][np.isinf(plain.X[:, 1])].all()  # without the zero coefficient those rows score


def test_cloglog_low_side_follows_the_oracle(gpu):
    """cloglog of -100 against -120: fp32 ties at 0, and so does the oracle's own float64 form —
    the float64 tie-break uses that form, so the label is the oracle's (the first class)."""
    case = E.low_side_case()
    c = CompiledPmml.from_string(case.probe.pmml())
    so, vo, _ = E.oracle(c, case.X)
    s, v, _ = _launch(PL.LinearPlan(c, gpu), _view(case.X, "contiguous", gpu), 3)
    assert np.array_equal(v, vo) and np.array_equal(s, so.astype(F32))


REG = [(5, lk, None) for lk in E.LINKS] + [(1, "none", None), (1, "exp", None), (63, "logit", None), (64, "none", None), (128, "exp", None)] \
    + [(5, "none", t) for t in E.TARGET_SHAPES] + [(5, "exp", "clip-rescale-round-default")]


@pytest.mark.parametrize("F,norm,target", REG, ids=[f"F{f}-{n}" + (f"-{t}" if t else "") for f, n, t in REG])
def test_linear_regression(gpu, F, norm, target):
    """EPI_AFFINE through every link, then every Target shape on values that sit on +-k.5, on the
    clip bounds and on -0.0; eta = +-inf and FLT_MAX cells; FLT_MAX + FLT_MAX is the fp32 rule."""
    case, c, ref = linear_case(0, F, norm, target=target)
    plan = PL.LinearPlan(c, gpu)
    assert plan.epi_args["mode"] == PL.EPI_AFFINE and ("tgt" in plan.epi_args) == bool(target)
    exact = norm == "none" or bool(E.TARGET_SHAPES.get(target, {}).get("cast"))
    if F == 1 and norm == "exp":
        # around ln(FLT_MAX): exp of the largest fp32 eta is beyond FLT_MAX (no prediction), exp of
        # its five predecessors is finite and stays one, within the bound like every other value
        edge = np.isin(case.eta[:, 0], E.EXP_EDGE)
        assert edge.sum() == 6 and ref["flagged"][edge].sum() == 1 and ref["valid"][edge].sum() == 5
    # none: FLT_MAX + FLT_MAX; exp: eta of 89 and more; a bounded link of an infinite eta is finite
    assert ref["flagged"].any() == (norm == "exp" or (norm == "none" and F > 1))
    for layout in LAYOUTS:
        s, v, _ = _launch(plan, _view(case.X, layout, gpu), 1)
        r = _check(f"{case.name} {layout}", s, v, None, ref, 0, norm, exact_values=exact)
    for n in ROW_COUNTS:
        s, v, _ = _launch(plan, _view(case.X[:n], "contiguous", gpu), 1)
        _check(f"{case.name} {n} rows", s, v, None, ref, 0, norm, slice(0, n), exact_values=exact)
    print(f"{case.name}: largest ratio {r:.3f} x 2^-24")


GLMS = {g.name: g for g in E.glm_cases()}


@pytest.mark.parametrize("name", list(GLMS))
def test_ordinal_and_binomial_glm(gpu, name):
    """EPI_CUMULATIVE (last cumulative value 1; cuts (0, 20): cumulative (0.5, saturated, 1), and
    (2e-9, 0.5, 1), where the fp32 tie of the last two classes goes to float64) and the binomial
    rule, through ``glm_pmml``'s grammar. The design lowering always wraps a GeneralRegressionModel,
    so the rows pass the derive kernel first (a plain copy of the covariates)."""
    g = GLMS[name]
    c = CompiledPmml.from_string(g.doc)
    plan = c.plan(gpu)
    assert type(plan).__name__ == "DerivedPlan" and type(plan.inner).__name__ == "LinearPlan"
    ref = g.reference(fp32_rule=True)
    assert not ref["flagged"].any()
    s, v, probs = _launch(plan, _view(g.X, "contiguous", gpu), g.K)
    r = _check(name, s, v, probs, ref, g.K, g.norm)
    print(f"{name}: largest ratio {r:.3f} x 2^-24")


# --------------------------------------------------------------------------- tree kernels

N_TREES, TREE_ROWS = 19, 257
# (id, depth, plan options, launch options)
TREE_PATHS = [
    ("perfect-narrow", 5, dict(layout="perfect", variant="narrow"), {}),
    ("perfect-wide", 5, dict(layout="perfect", variant="wide"), {}),
    ("pointer", 9, dict(layout="pointer"), {}),
    ("general", 5, dict(layout="general"), {}),
    ("hybrid", 9, dict(layout="hybrid", hybrid_tail="compact"), {}),
    ("lds-forest", 9, dict(layout="pointer", node_format="lds"), {}),
    ("pointer-compact", 9, dict(layout="pointer", node_format="compact"), {}),
    ("pointer-super", 9, dict(layout="pointer", node_format="super"), {}),
    ("pointer-rank3", 9, dict(layout="pointer", node_format="rank3"), {}),
    ("perfect-splits4", 5, dict(layout="perfect", variant="narrow"), dict(splits=4)),
    ("pointer-splits4", 9, dict(layout="pointer"), dict(splits=4)),
]
HOST_ONLY = {("multiclass", "general")}  # K-class chains over the predicate-VM layout are refused at lowering
NO_NULL = {"pointer-rank3"}  # the rank3 records carry no null-on-missing flag: those documents use defaultChild


@functools.lru_cache(maxsize=None)
def tree_case(objective: str, depth: int, target: str = "", null: bool = True):
    """Integer leaves -2..2 (19 trees: sums within +-38, many on 0 and on the clip bounds), every cell
    a split constant +-2 ulps or a special value. Oracle scores, validity, probabilities: once."""
    txt = gbdt_pmml(n_trees=N_TREES, depth=depth, n_features=8, seed=21, p_split=0.9 if depth <= 6 else 0.75,
                    objective=objective)
    txt = B.integer_leaves(B.mix_mutants(txt), modulus=5)
    if null:
        txt = B.null_prediction(txt)
    if target:
        txt = set_target(txt, **E.TARGET_SHAPES[target])
    c = CompiledPmml.from_string(txt)
    X = B.boundary_matrix(B.split_cuts(txt, 8), TREE_ROWS, seed=depth)
    s, v, probs = E.oracle(c, X)
    assert v.any() and (not v.all() or not null or "default" in E.TARGET_SHAPES.get(target, {}))
    return c, X, s, v, probs


def _exact_accumulators(plan):
    """The affine map of the plan keeps integer leaf sums exact fp32 numbers (multiples of 1/2)."""
    a, b = plan.epi_args.get("a", 1.0), plan.epi_args.get("b", 0.0)
    assert a in (1.0, 0.5, 2.0) and b * 2 == round(b * 2), (a, b)


def _tree_launch(plan, X, C, launch):
    Xt = torch.from_numpy(np.array(X, dtype=F32)).to(plan.device)
    s, v = plan.alloc_outputs(len(X))
    probs = torch.full((len(X), C), -7.0, dtype=torch.float32, device=plan.device) if C else None
    plan.launch(Xt, s, v, probs=probs, **launch)
    torch.cuda.synchronize()
    return s.cpu().numpy(), v.cpu().numpy().astype(bool), None if probs is None else probs.cpu().numpy()


def test_multiclass_chain_over_the_general_layout_is_refused():
    c = tree_case("multiclass", 5)[0]
    with lowering_dry_run(), pytest.raises(PL.NotLowerable):
        PL.TreePlan(c, torch.device("cpu"), layout="general")


CHAINS = [(p, o) for o in ("binary", "multiclass") for p in TREE_PATHS if (o, p[0]) not in HOST_ONLY]


@pytest.mark.parametrize("path,objective", CHAINS, ids=[f"{p[0]}-{o}" for p, o in CHAINS])
def test_tree_chain_epilogues(gpu, path, objective):
    """EPI_LOGISTIC2 (binary chain) and EPI_SOFTMAX with ``probs=`` (3-class chain) behind every
    accumulator accessor: labels and validity equal to the oracle on all 257 rows, probabilities
    within the logit / softmax bound. The 3-class chain accumulates class slots with one value
    per leaf: the compact node formats (hybrid tail, compact, lds, super, rank3) keep that value
    in the leaf slot itself, and their kernels must not read it as a row of the leaf table."""
    name, depth, opts, launch = path
    c, X, so, vo, po = tree_case(objective, depth, null=name not in NO_NULL)
    plan = PL.TreePlan(c, gpu, **opts)
    _exact_accumulators(plan)
    C = 2 if objective == "binary" else 3
    assert plan.epi_args["mode"] == (PL.EPI_LOGISTIC2 if C == 2 else PL.EPI_SOFTMAX)
    s, v, probs = _tree_launch(plan, X, C, launch)
    assert np.array_equal(v, vo), f"validity differs on rows {np.flatnonzero(v != vo)[:8]}"
    assert np.array_equal(s[vo], so[vo].astype(F32))
    key = "logit" if C == 2 else "softmax"
    r = _ratio(key, probs[vo], po[vo], what=f"{name} {objective}")
    print(f"{name} {objective}: largest ratio {r:.3f} x 2^-24")
    assert r <= E.C_BOUND[key]


@pytest.mark.parametrize("path", TREE_PATHS, ids=[p[0] for p in TREE_PATHS])
def test_tree_regression_under_every_target_shape(gpu, path):
    """Integer leaf sums through ``apply_target`` (and the split-reduction epilogue): every score
    is exact, so all of them compare bit for bit, defaults on the rows without a prediction."""
    name, depth, opts, launch = path
    for target in E.TARGET_SHAPES:
        c, X, so, vo, _ = tree_case("regression", depth, target, null=name not in NO_NULL)
        plan = PL.TreePlan(c, gpu, **opts)
        _exact_accumulators(plan)
        assert "tgt" in plan.epi_args
        s, v, _ = _tree_launch(plan, X, 0, launch)
        assert np.array_equal(v, vo), f"{name} {target}: validity"
        assert np.array_equal(X_.bits(s[vo]), X_.bits(so[vo])), f"{name} {target}: scores"


# --------------------------------------------------------------------------- Target stage of the other heads

HEAD_TARGETS = ("clip-round", "clip-rescale-floor", "rescale-ceiling", "round-default", "clip-rescale-round-default")


def _head(gpu, txt, X, target, **opts):
    c = CompiledPmml.from_string(set_target(txt, **E.TARGET_SHAPES[target]))
    so, vo, _ = E.oracle(c, X)
    plan = c.plan(gpu, **opts)
    s, v = plan.score(np.array(X))
    torch.cuda.synchronize()
    s, v = s.cpu().numpy(), v.cpu().numpy().astype(bool)
    assert np.array_equal(v, vo), f"{target}: validity differs on {(v != vo).sum()} rows"
    assert np.array_equal(X_.bits(s[vo]), X_.bits(so[vo])), f"{target}: scores differ"
    return plan, so, vo


@pytest.mark.parametrize("kind", ["fused", "gemm"])
def test_mlp_regression_head_target(gpu, kind):
    layers, cls, txt = X_.network(X_.FUSED_SHAPES["17-33-1"], 1)
    X = X_.probe_matrix(257, 17, seed=3)
    X_.nn_reference(layers, X)  # asserts the exactness guard
    for target in HEAD_TARGETS:
        plan, so, vo = _head(gpu, txt, X, target, **({} if kind == "fused" else {"mlp_impl": "gemm"}))
        assert plan.kind == ("mlp" if kind == "fused" else "mlp_gemm")
        assert len(np.unique(so[vo])) > 2 and (not vo.all() or "default" in target)


@pytest.mark.parametrize("impl", ["fused", "wide", "gemm"])
def test_svm_regression_head_target(gpu, impl):
    probe, _ = X_.svm_probe("mfma-reg")
    X = X_.svm_matrix(257, probe.F)
    probe.reference(X)
    for target in HEAD_TARGETS:
        _, so, vo = _head(gpu, probe.pmml(), X, target, svm_impl=impl)
        assert len(np.unique(so[vo])) > 2


@pytest.mark.parametrize("N,k,method,metric,F", [(65, 9, "median", "squaredEuclidean", 3),
                                                 (65, 2, "average", "squaredEuclidean", 5)])
def test_knn_regression_head_target(gpu, N, k, method, metric, F):
    """``average`` over 2 neighbours puts values on k.5: the round-half-up rows of the k-NN head."""
    inst, targets, classes = X_.knn_probe(N, k, method, metric, F)
    txt = X_.knn_pmml_exact(inst, targets, k, method, metric, classes)
    X = X_.center_matrix(inst, 192, seed=N)
    for target in HEAD_TARGETS:
        _, so, vo = _head(gpu, txt, X, target)
        assert len(np.unique(so[vo])) > 2


def test_print_measured_ratios():
    """Last in the file: the largest ratio per link seen by the tests above (docs/PARITY.md)."""
    for k, (r, where) in sorted(RATIOS.items()):
        print(f"measured ratio {k}: {r:.4f} x 2^-24 (bound {E.C_BOUND[k]}) {where}")
