"""Every kernel path on inputs that sit on the model's own boundaries, against the float64 oracle
(GPU twin of tests/test_boundary_inputs.py): validity exact, regression scores bit for bit (integer
leaves, see tests/_boundary.py), vote labels equal, no row excluded.

Shapes: 2049 rows (a ragged last tile and a 1-row tile), 19 trees (one full and one partial 16-walk
group), F = 8 (40 for the wide PERFECT kernel, 65 where the walk kernels leave the features in
global memory), depth 5 for PERFECT and 9 for the pointer family
(past the 5 LDS-staged LTOP levels, the hybrid head and the rank3 / super multi-level records).
Each tree of a document takes another mutant (operator pair, child order, fp32 / decimal
thresholds), and every cell of the input is a split constant +-2 ulps or a special value."""

import functools

import numpy as np
import pytest
import torch

from tests import _boundary as B
from tests import _prep_grid as G

from flink_jpmml_amd.bench.synth import gbdt_pmml, kmeans_pmml, random_forest_pmml
from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import lowering_dry_run

F32 = np.float32
ROWS = 2049
N_TREES = 19
NS = "http://www.dmg.org/PMML-4_4"


@functools.lru_cache(maxsize=None)
def tree_case(model: str, depth: int, F: int, missing: str, leaf_modulus: int = B.LEAF_PRIME):
    """(document, compiled, X, oracle scores, oracle validity) — built once, shared, never changed."""
    p_split = 0.9 if depth <= 6 else 0.75
    if model == "gbdt":
        txt = gbdt_pmml(n_trees=N_TREES, depth=depth, n_features=F, seed=21, p_split=p_split)
        txt = B.integer_leaves(B.mix_mutants(txt), modulus=leaf_modulus)
    else:
        txt = random_forest_pmml(n_trees=N_TREES, depth=depth, n_features=F, n_classes=3, seed=22, p_split=p_split)
        txt = B.integer_leaves(B.mix_mutants(txt), labels=("0", "1", "2"))
    if missing == "nullPrediction":
        txt = B.null_prediction(txt)
    c = CompiledPmml.from_string(txt)
    X = B.boundary_matrix(B.split_cuts(txt, F), ROWS, seed=depth + F)
    ref, vref = c.score_matrix_oracle(X)
    if model == "gbdt":
        B.assert_fp32_exact(ref, vref)
    assert vref.any() and (missing == "defaultChild" or not vref.all())
    for a in (X, ref, vref):
        a.setflags(write=False)
    return txt, c, X, ref, vref


def _score(plan, X, **launch):
    if launch:
        Xt = torch.from_numpy(np.array(X, dtype=F32)).to(plan.device)
        s, v = plan.alloc_outputs(len(X))
        plan.launch(Xt, s, v, **launch)
    else:
        s, v = plan.score(np.array(X))
    torch.cuda.synchronize()
    return s.cpu().numpy(), v.cpu().numpy().astype(bool)


def _assert_same(s, v, ref, vref, what):
    assert np.array_equal(v, vref), f"{what}: validity differs on {(v != vref).sum()} of {len(v)} rows"
    bad = np.nonzero(s[vref].astype(F32) != ref[vref].astype(F32))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {int(vref.sum())} valid rows differ from the oracle"


# (id, depth, F, plan options, launch options, models, variant bits that must be set)
BOTH = ("gbdt", "rf")
PATHS = [
    ("perfect-narrow", 5, 8, dict(layout="perfect", variant="narrow"), {}, BOTH, 0),
    ("perfect-wide-nan-auto", 5, 40, dict(layout="perfect", variant="wide", nan_mode="auto"), {}, BOTH, 0),
    ("perfect-wide-nan-off", 5, 40, dict(layout="perfect", variant="wide", nan_mode="off"), {}, BOTH, 0),
    ("perfect-wide-f8", 5, 8, dict(layout="perfect", variant="wide"), {}, BOTH, 0),
    ("pointer-clamped", 9, 8, dict(layout="pointer", pointer_load="clamped"), {}, BOTH, 0),
    ("pointer-masked", 9, 8, dict(layout="pointer", pointer_load="masked"), {}, BOTH, PL.VAR_POINTER_MASKED),
    ("pointer-uskip", 9, 8, dict(layout="pointer", pointer_load="uskip"), {}, BOTH, PL.VAR_POINTER_USKIP),
    ("pointer-peel-dfs", 9, 8, dict(layout="pointer", pointer_load="peel", node_order="dfs"), {}, BOTH,
     PL.VAR_POINTER_PEEL),
    ("pointer-ltop", 9, 8, dict(layout="pointer", pointer_load="ltop"), {}, BOTH, PL.VAR_POINTER_LTOP),
    ("pointer-refill", 9, 8, dict(layout="pointer", pointer_schedule="refill"), {}, BOTH, PL.VAR_POINTER_REFILL),
    ("pointer-inline", 9, 8, dict(layout="pointer", pointer_leaf="inline"), {}, BOTH, PL.VAR_POINTER_INLINE),
    ("pointer-compact", 9, 8, dict(layout="pointer", node_format="compact"), {}, BOTH, PL.VAR_POINTER_COMPACT),
    ("pointer-super", 9, 8, dict(layout="pointer", node_format="super"), {}, BOTH, PL.VAR_POINTER_SUPER),
    ("pointer-rank3", 9, 8, dict(layout="pointer", node_format="rank3"), {}, BOTH, PL.VAR_POINTER_RANK3),
    ("pointer-lds", 9, 8, dict(layout="pointer", node_format="lds"), {}, BOTH, PL.VAR_POINTER_LDS),
    ("pointer-ilp4", 9, 8, dict(layout="pointer", pointer_ilp=4), {}, BOTH, 0),
    ("pointer-ilp16", 9, 8, dict(layout="pointer", pointer_ilp=16), {}, BOTH, 0),
    ("pointer-xcd", 9, 8, dict(layout="pointer", xcd_split="on"), {}, BOTH, 0),
    ("hybrid-compact-tail", 9, 8, dict(layout="hybrid", hybrid_tail="compact"), {}, BOTH, 0),
    ("hybrid-wide-tail", 9, 8, dict(layout="hybrid", hybrid_tail="wide"), {}, BOTH, 0),
    ("general", 5, 8, dict(layout="general"), {}, BOTH, 0),
    ("perfect-splits4", 5, 8, dict(layout="perfect", variant="narrow"), dict(splits=4), BOTH, 0),
    ("pointer-splits4", 9, 8, dict(layout="pointer"), dict(splits=4), BOTH, 0),
]
# PATHS above is also the grid tests/test_tree_plan_pins.py pins against its recorded fixture, so
# it only grows together with that fixture; the rows below run through the same two tests here.
MORE_PATHS = [
    # F = 65: features stay in global memory (the walk kernels' lazy per-read preparation)
    ("pointer-clamped-f65", 9, 65, dict(layout="pointer", pointer_load="clamped"), {}, BOTH, 0),
    ("pointer-refill-f65", 9, 65, dict(layout="pointer", pointer_schedule="refill"), {}, BOTH, PL.VAR_POINTER_REFILL),
    ("pointer-inline-f65", 9, 65, dict(layout="pointer", pointer_leaf="inline"), {}, BOTH, PL.VAR_POINTER_INLINE),
    ("hybrid-compact-tail-f65", 9, 65, dict(layout="hybrid", hybrid_tail="compact"), {}, BOTH, 0),
    ("hybrid-wide-tail-f65", 9, 65, dict(layout="hybrid", hybrid_tail="wide"), {}, BOTH, 0),
    ("general-f65", 5, 65, dict(layout="general"), {}, BOTH, 0),
    # split partials of the other node formats (pointer-splits4 covers the plain pointer walk)
    ("pointer-compact-splits4", 9, 8, dict(layout="pointer", node_format="compact"), dict(splits=4), BOTH,
     PL.VAR_POINTER_COMPACT),
    ("pointer-super-splits4", 9, 8, dict(layout="pointer", node_format="super"), dict(splits=4), BOTH,
     PL.VAR_POINTER_SUPER),
    ("pointer-rank3-splits4", 9, 8, dict(layout="pointer", node_format="rank3"), dict(splits=4), BOTH,
     PL.VAR_POINTER_RANK3),
    ("pointer-refill-splits4", 9, 8, dict(layout="pointer", pointer_schedule="refill"), dict(splits=4), BOTH,
     PL.VAR_POINTER_REFILL),
    ("hybrid-compact-tail-splits4", 9, 8, dict(layout="hybrid", hybrid_tail="compact"), dict(splits=4), BOTH, 0),
    ("hybrid-wide-tail-splits4", 9, 8, dict(layout="hybrid", hybrid_tail="wide"), dict(splits=4), BOTH, 0),
]
MISSING = ["defaultChild", "nullPrediction"]
ALL_PATHS = PATHS + MORE_PATHS
NO_NULL = {"pointer-rank3", "pointer-rank3-splits4"}  # the rank3 records carry no null-on-missing flag: refused at lowering
CASES = [(p, m) for p in ALL_PATHS for m in MISSING if not (m == "nullPrediction" and p[0] in NO_NULL)]


def _lowers(c, opts):
    try:
        with lowering_dry_run():
            return PL.TreePlan(c, torch.device("cpu"), **opts)
    except PL.NotLowerable:
        return None


@pytest.mark.parametrize("path", ALL_PATHS, ids=[p[0] for p in ALL_PATHS])
def test_every_kernel_path_lowers_as_named(path):
    """CPU: each case's options select the kernel it is named after (no silent other path), for
    both models under both missing-value strategies."""
    name, depth, F, opts, _, models, bits = path
    for model, missing in [(a, b) for a in models for b in MISSING]:
        _, c, _, _, _ = tree_case(model, depth, F, missing)
        plan = _lowers(c, opts)
        if missing == "nullPrediction" and name in NO_NULL:
            assert plan is None
            continue
        assert plan is not None, (name, model, missing)
        assert plan.layout == opts["layout"] and plan.n_trees >= N_TREES
        assert plan.variant & bits == bits, (name, plan.variant)
        if opts.get("variant") == "wide":
            assert plan.variant & 3 in (1, 2)
            assert (plan.blob_nan is not None) == (opts.get("nan_mode", "auto") == "auto" and missing == "defaultChild")
        if opts.get("variant") == "narrow":
            assert plan.variant & 3 == 0
        if opts.get("xcd_split") == "on":
            assert plan.xcd_split == PL.XCD_SLICES and plan._auto_splits(ROWS) > 1
        if F > 64:  # the kernels stage features in LDS up to 64 columns: these stay in global memory
            assert plan.n_features == F
            # what a node reads is then a column index below F, never an LDS byte offset (f * 1024)
            u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
            if plan.layout == "pointer":
                fields = u32(plan.blob).reshape(-1, 4)[:, 1] & 0xFFFF
            elif plan.layout == "hybrid":
                NI = (1 << plan.head_depth) - 1
                fields = u32(plan.heads).reshape(plan.n_trees, plan.rec_words)[:, 1:2 * NI:2].reshape(-1) & 0xFFFF
                wide = plan.tail_format != 0
                tail = u32(plan.blob).reshape(-1, 4 if wide else 2)[:, 1] & (0xFFFF if wide else 0xFF)
                fields = np.concatenate([fields, tail])
            else:  # general: predicate rows {op | neg << 8, field, ..}; ops 3..7 read a field
                preds = u32(plan.preds).reshape(-1, 4)
                fields = preds[np.isin(preds[:, 0] & 0xFF, (3, 4, 5, 6, 7)), 1]
            assert fields.size and 8 <= int(fields.max()) < F


@pytest.mark.gpu
@pytest.mark.parametrize("path,missing", CASES, ids=[f"{p[0]}-{m}" for p, m in CASES])
def test_kernel_path_on_boundary_inputs(gpu, path, missing):
    """Regression GBDT (bit-exact scores) and 3-class vote forest (equal labels) through one
    kernel path; validity exact; all 2049 rows."""
    name, depth, F, opts, launch, models, bits = path
    for model in models:
        _, c, X, ref, vref = tree_case(model, depth, F, missing)
        plan = PL.TreePlan(c, gpu, **opts)
        assert plan.variant & bits == bits
        s, v = _score(plan, X, **launch)
        _assert_same(s, v, ref, vref, f"{name} {model} {missing}")


# ------------------------------------------------- leaf payloads of the lock-step pointer walk
#
# pointer_walk (tree.hip) adds a GENERAL leaf in one of four ways. Where the GPU suite reaches them
# (plans traced through the whole suite):
#   * one-hot {class, weight} pairs: every 3-class vote forest on the lock-step path, e.g.
#     test_kernel_path_on_boundary_inputs[pointer-clamped / -masked / -uskip / -peel-dfs / -ltop];
#   * runtime-P loop: P = 1 class slots, test_gpu_epilogue.py::test_tree_chain_epilogues[pointer-multiclass];
#   * dense P == 3 gather: only behind inline leaves (pointer-inline rows, test_inline_leaves.py), where
#     all but single-leaf trees skip it, and in members of segmented plans (test_gpu_segment_reduce.py);
#   * dense P == 2 gather: nowhere.
# The two dense gathers get the cases below: an `average` forest whose leaves carry integer class
# payloads (ScoreDistribution probability = 0..6, not one-hot), 16 trees, so every class mean is a
# sum of integers below 2**7 times 2**-4: exact in fp32 and in the float64 oracle alike.
DENSE_TREES = 16
DENSE_PATHS = [
    ("clamped", dict(layout="pointer", pointer_load="clamped"), {}),
    ("uskip", dict(layout="pointer", pointer_load="uskip"), {}),
    ("splits4", dict(layout="pointer"), dict(splits=4)),
]


@functools.lru_cache(maxsize=None)
def dense_case(n_classes: int, missing: str):
    """(compiled, X, oracle labels, validity, class means) of the integer-payload average forest."""
    import re

    from tests import _epilogue_cases as E

    txt = random_forest_pmml(n_trees=DENSE_TREES, depth=9, n_features=8, n_classes=n_classes, seed=23, p_split=0.75)
    txt = B.mix_mutants(txt).replace('multipleModelMethod="majorityVote"', 'multipleModelMethod="average"')
    count = [0]

    def leaf(m):
        k = count[0]
        count[0] += 1
        dist = "".join(f'<ScoreDistribution value="{c}" recordCount="1" probability="{(k * (c + 2) + c) % 7}"/>'
                       for c in range(n_classes))
        return m.group(1) + m.group(2) + dist + m.group(3)

    txt, n = re.subn(r'(<Node id="\d+" score="[^"]+">)(<SimplePredicate [^>]*/>)(</Node>)', leaf, txt)
    assert n > DENSE_TREES
    if missing == "nullPrediction":
        txt = B.null_prediction(txt)
    c = CompiledPmml.from_string(txt)
    X = B.boundary_matrix(B.split_cuts(txt, 8), ROWS, seed=n_classes)
    ref, vref, probs = E.oracle(c, X)
    assert vref.any() and (missing == "defaultChild" or not vref.all())
    sums = probs[vref] * DENSE_TREES
    assert np.array_equal(sums, np.round(sums)) and sums.max() < 2 ** 7  # integer sums: fp32-exact means
    assert (np.sort(sums, axis=1)[:, :-1] > 0).any()  # not one-hot: more than one class has mass
    for a in (X, ref, vref, probs):
        a.setflags(write=False)
    return c, X, ref, vref, probs


@pytest.mark.parametrize("n_classes", [3, 2])
def test_dense_leaf_payloads_lower_to_the_dense_gathers(n_classes):
    """CPU: the cases below take pointer_walk's dense ``P == 3`` / ``P == 2`` branch (GENERAL, P = the
    class count, no one-hot pairs, the lock-step kernel)."""
    for missing in MISSING:
        c = dense_case(n_classes, missing)[0]
        for name, opts, _ in DENSE_PATHS:
            plan = _lowers(c, opts)
            assert plan is not None and plan.layout == "pointer" and plan.general == 1, (name, missing)
            assert plan.P == n_classes and plan.C == n_classes and not plan.leaf_onehot
            # tree_pointer_kernel (pointer_walk) with the leaves in the leaf table, not inline
            assert plan.variant in (0, PL.VAR_POINTER_USKIP, PL.VAR_POINTER_LTOP)


@pytest.mark.gpu
@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("n_classes", [3, 2])
def test_dense_leaf_payloads_on_boundary_inputs(gpu, n_classes, missing):
    """The dense gathers, bit for bit: every class mean equals the oracle's on every valid row,
    validity exact, labels equal wherever the oracle's best class is not tied."""
    c, X, ref, vref, probs = dense_case(n_classes, missing)
    top = np.sort(probs[vref], axis=1)
    clear = top[:, -1] > top[:, -2]
    assert clear.sum() >= vref.sum() // 2
    for name, opts, launch in DENSE_PATHS:
        plan = PL.TreePlan(c, gpu, **opts)
        assert plan.P == n_classes and not plan.leaf_onehot
        Xt = torch.from_numpy(np.array(X, dtype=F32)).to(gpu)
        s, v = plan.alloc_outputs(len(X))
        p = torch.full((len(X), n_classes), -7.0, dtype=torch.float32, device=gpu)
        plan.launch(Xt, s, v, probs=p, **launch)
        torch.cuda.synchronize()
        s, v, p = s.cpu().numpy(), v.cpu().numpy().astype(bool), p.cpu().numpy()
        what = f"dense P = {n_classes} {name} {missing}"
        assert np.array_equal(v, vref), f"{what}: validity differs on {(v != vref).sum()} rows"
        assert np.array_equal(p[vref], probs[vref].astype(F32)), f"{what}: class means differ from the oracle"
        assert np.array_equal(s[vref][clear].astype(F32), ref[vref][clear].astype(F32)), f"{what}: labels differ"


@pytest.mark.gpu
@pytest.mark.parametrize("missing", MISSING)
def test_fp8_leaves_on_boundary_inputs(gpu, missing):
    """fp8 leaves (e4m3 leaf pairs in the last-level metas, one global scale). Leaves are the
    integers -7..7, scale = 7 / 448 = 1 / 64: every de-quantised packed leaf is its integer again,
    so the smallest sibling-leaf gap of the de-quantised leaves is 1.0 and the tolerance half of
    it, 0.5 — computed below from the packed blob, not from any kernel output. One walk that ends
    on the wrong sibling moves the sum by at least that gap. (Pairs with equal bytes are the
    padding under a leaf that sits above the last level: both slots hold that one leaf. Two real
    sibling leaves never share a byte here, since every leaf de-quantises to its own integer and
    siblings are consecutive counter values.)"""
    _, c, X, ref, vref = tree_case("gbdt", 5, 8, missing, 15)
    plan = PL.TreePlan(c, gpu, precision="fp8")
    D = plan.depth
    NI = (1 << D) - 1
    blob = plan.blob.cpu().numpy().view(np.uint32).reshape(plan.n_trees, plan.rec_words)
    meta = blob[:, 1:2 * NI:2][:, NI // 2:]  # last-level nodes
    scale = plan.epi_args["a"] / plan.full_epi.get("a", 1.0)
    left = PL.dequantize_fp8(((meta >> 16) & 0xFF).astype(np.uint8).reshape(-1)) * scale
    right = PL.dequantize_fp8((meta >> 24).astype(np.uint8).reshape(-1)) * scale
    both = np.concatenate([left, right])
    assert np.array_equal(both, np.round(both)) and np.abs(both).max() == 7  # exact integers -7..7
    real = left != right
    assert real.sum() >= plan.n_trees  # every tree (forced root split, p_split 0.9) has last-level sibling leaves
    gap = float(np.min(np.abs(left - right)[real]))
    print(f"fp8: scale {scale!r}, smallest sibling-leaf gap {gap!r}, tolerance {gap / 2!r}")
    assert gap >= 1.0
    s, v = _score(plan, X)
    assert np.array_equal(v, vref)
    err = np.abs(s[vref].astype(np.float64) - ref[vref])
    print(f"fp8: max |device - oracle| = {err.max()!r}")
    assert err.max() <= gap / 2


# --------------------------------------------------------------------------- field preparation


@functools.lru_cache(maxsize=None)
def prep_case(model: str, family: str, dtype: str):
    n_cells = len(G.family_document(gbdt_pmml(n_trees=1, depth=1, n_features=64, seed=0), family, dtype)[1])
    F = max(n_cells, 4)
    if model == "gbdt":
        base = B.integer_leaves(gbdt_pmml(n_trees=N_TREES, depth=4, n_features=F, seed=31))
    else:
        base = kmeans_pmml(n_clusters=5, n_features=F, seed=32)
    txt, cells = G.family_document(base, family, dtype)
    c = CompiledPmml.from_string(txt)
    X = G.family_inputs(cells, F)
    ref, vref = c.score_matrix_oracle(X.astype(np.float64))
    assert vref.any() and (family == "outliers" or not vref.all())  # outliers never reject a row
    return c, X, ref, vref, txt


def _assert_near_minimum(txt, c, X, s, ref, vref):
    """k-means labels: equal to the oracle's, or — where fp32 cannot resolve the argmin — a cluster
    whose float64 distance is within the fp32 error of the minimum. Bound: the kernels may expand
    ``|x - c|**2 = |x|**2 - 2 x.c + |c|**2``; each of the three sums of F products carries a
    relative error of at most (F + 1) * 2**-24 of its magnitude, which is at most
    ``|x|**2 + |c|**2`` (2 |x.c| included), so ``|d32 - d64| <= 3 * (F + 1) * 2**-24 * 2 * (|x|**2 +
    |c|**2)`` per distance, and twice that between two of them. At ordinary inputs (|x| ~ 1) that
    is ~1e-5 against centre separations of order 1; at x = 2**24 it exceeds every separation."""
    import re

    centres = np.array([[float(t) for t in m.split()] for m in re.findall(r'type="real">([^<]+)</Array>', txt)])
    P, ok = c.prepare(X.astype(np.float64))
    assert np.array_equal(ok[vref], np.ones(int(vref.sum()), bool))
    P = P[vref]
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((P[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
        Fn = P.shape[1]
        tol = 2 * 3 * (Fn + 1) * 2.0 ** -24 * 2 * ((P ** 2).sum(axis=1) + (centres ** 2).sum(axis=1).max())
        got, want = s[vref].astype(int) - 1, ref[vref].astype(int) - 1  # cluster ids are 1-based
        rows = np.arange(len(P))
        assert np.array_equal(d.argmin(axis=1)[np.isfinite(d).all(axis=1)], want[np.isfinite(d).all(axis=1)])
        near = d[rows, got] - d[rows, want] <= tol
    same = got == want
    assert (same | near).all(), f"{(~(same | near)).sum()} labels are not a minimum within the fp32 bound"
    ordinary = np.abs(P).max(axis=1) <= 1000
    assert ordinary.sum() >= len(P) // 4 and same[ordinary].all()  # only huge inputs may use the bound


@pytest.mark.parametrize("family,dtype", G.FAMILIES)
def test_field_preparation_family_twin(family, dtype):
    """CPU: the family documents the GPU tests score, through the ``prep_value`` twin."""
    from test_boundary_inputs import emulate_prep

    c, X, _, vref, _ = prep_case("gbdt", family, dtype)
    raw, any_prep = PL.build_field_prep(c, c.active_fields)
    assert any_prep
    P, ok = c.prepare(X.astype(np.float64))
    got, bad = emulate_prep(raw, X)
    assert np.array_equal(ok, ~bad) and np.array_equal(ok, vref)
    assert np.array_equal(got[ok], P[ok].astype(F32), equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("family,dtype", G.FAMILIES)
@pytest.mark.parametrize("model", ["gbdt", "kmeans"])
def test_field_preparation_on_the_bounds(gpu, model, family, dtype):
    """``prep_value`` inside the tree kernels' and ``cluster.hip``'s tile loaders: every treatment
    of the family at its bounds +-{0, 1, 2} ulps, +-inf, NaN. Validity is the oracle's row for row;
    the GBDT's integer-leaf scores bit for bit; k-means labels equal (at inputs like 2**24, where
    fp32 distances cannot tell the centres apart: a minimum within the fp32 error bound)."""
    c, X, ref, vref, txt = prep_case(model, family, dtype)
    plan = c.plan(gpu)
    assert getattr(plan, "prep", None) is not None
    s, v = _score(plan, X)
    if model == "gbdt":
        _assert_same(s, v, ref, vref, f"{model} {family} {dtype}")
    else:
        assert np.array_equal(v, vref), f"validity differs on {(v != vref).sum()} rows"
        _assert_near_minimum(txt, c, X, s, ref, vref)


# --------------------------------------------------------------------------- folded derived fields


@pytest.mark.gpu
def test_folded_fields_at_their_cuts_and_at_infinity_on_gpu(gpu):
    from test_boundary_inputs import folded_case

    _, c, X = folded_case(rows=ROWS)
    ref, vref = c.score_matrix_oracle(X)
    B.assert_fp32_exact(ref, vref)
    plan = c.plan(gpu)
    assert type(plan).__name__ == "TreePlan"  # folded: no derive pass
    s, v = _score(plan, X)
    _assert_same(s, v, ref, vref, "folded")
    Xi = np.array(B.boundary_matrix([[0.0]] * 8, 16 * 257, 0, specials=False))
    for k, value in enumerate((np.inf, -np.inf)):
        for j in range(8):
            sl = slice((8 * k + j) * 257, (8 * k + j + 1) * 257)  # a tile and a row of the next per column
            Xi[sl, j] = value
            Xi[sl, (j + 1) % 8] = X[:257, (j + 1) % 8]
    ref, vref = c.score_matrix_oracle(Xi)
    s, v = _score(plan, Xi)
    _assert_same(s, v, ref, vref, "folded, one column at +-inf")


# --------------------------------------------------------------------------- derive.hip


def discretize_doc(dtype: str) -> str:
    """Eight ``Discretize`` fields (each closure on two inputs, two adjacent bins sharing an edge)
    under a RegressionModel with coefficients 5**i: bin values 1..4 make the score an exact fp32
    integer sum that names every field's bin."""
    dd = "".join(f'<DataField name="{n}" optype="continuous" dataType="{dtype}"/>' for n in "ab")
    dd += '<DataField name="y" optype="continuous" dataType="double"/>'
    ders, names = [], []
    for cl in G.CLOSURES:
        for fld, (lo, hi) in (("a", (0.3, 0.7)), ("b", (-0.75, 0.5))):
            names.append(f"d_{cl}_{fld}")
            ders.append(
                f'<DerivedField name="{names[-1]}" optype="continuous" dataType="integer"><Discretize field="{fld}" '
                f'mapMissingTo="4" defaultValue="2"><DiscretizeBin binValue="1"><Interval closure="{cl}" '
                f'leftMargin="{lo}" rightMargin="{hi}"/></DiscretizeBin><DiscretizeBin binValue="3"><Interval '
                f'closure="{cl}" leftMargin="{hi}" rightMargin="5"/></DiscretizeBin></Discretize></DerivedField>')
    preds = "".join(f'<NumericPredictor name="{n}" coefficient="{5 ** i}"/>' for i, n in enumerate(names))
    return (f'<PMML version="4.4" xmlns="{NS}"><DataDictionary>{dd}</DataDictionary><TransformationDictionary>'
            f'{"".join(ders)}</TransformationDictionary><RegressionModel functionName="regression"><MiningSchema>'
            '<MiningField name="y" usageType="target"/><MiningField name="a"/><MiningField name="b"/></MiningSchema>'
            f'<RegressionTable intercept="0.5">{preds}</RegressionTable></RegressionModel></PMML>')


DERIVE_CUTS = [[0.3, 0.7, 5.0], [-0.75, 0.5, 5.0]]


def norm_doc(dtype: str) -> str:
    """``NormContinuous`` with ``outliers="asMissingValues"``: outside the outer knots the value is
    missing and maps to 64, inside it lies in [0, 1] — a jump of 63 at each outer knot."""
    dd = "".join(f'<DataField name="{n}" optype="continuous" dataType="{dtype}"/>' for n in "ab")
    dd += '<DataField name="y" optype="continuous" dataType="double"/>'
    ders = "".join(
        f'<DerivedField name="n_{fld}" optype="continuous" dataType="double"><NormContinuous field="{fld}" '
        f'outliers="asMissingValues" mapMissingTo="64"><LinearNorm orig="{k[0]}" norm="0"/><LinearNorm orig="{k[1]}" '
        f'norm="0.5"/><LinearNorm orig="{k[2]}" norm="1"/></NormContinuous></DerivedField>'
        for fld, k in (("a", DERIVE_CUTS[0]), ("b", DERIVE_CUTS[1])))
    return (f'<PMML version="4.4" xmlns="{NS}"><DataDictionary>{dd}</DataDictionary><TransformationDictionary>'
            f'{ders}</TransformationDictionary><RegressionModel functionName="regression"><MiningSchema>'
            '<MiningField name="y" usageType="target"/><MiningField name="a"/><MiningField name="b"/></MiningSchema>'
            '<RegressionTable intercept="0"><NumericPredictor name="n_a" coefficient="1"/>'
            '<NumericPredictor name="n_b" coefficient="256"/></RegressionTable></RegressionModel></PMML>')


def _derive_inputs():
    X = np.array(B.boundary_matrix(DERIVE_CUTS, 1025, 4))
    X[np.isinf(X) | (np.abs(X) > 1e30)] = F32(0.25)  # NormContinuous extrapolates nothing here; keep sums finite
    return X


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_derive_program_twin_on_the_edges(dtype):
    """CPU: the derive program's numpy emulation on the edges +-2 ulps, exact for every bin."""
    from flink_jpmml_amd.runtime.derive import emulate, plan_field_layout

    c = CompiledPmml.from_string(discretize_doc(dtype))
    prog = plan_field_layout(c).program
    X = _derive_inputs()
    P, ok = c.prepare(X.astype(np.float64))
    assert ok.all()
    got, cols = emulate(prog, P), c.columns(P)
    for j, name in enumerate(prog.selected):
        assert np.array_equal(got[:, j], cols.get(name).astype(F32)), name


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_derive_kernel_on_the_edges(gpu, dtype):
    """``derive.hip``: ``Discretize`` with all four closures, inputs at the bin edges +-2 ulps
    (bit-exact: the score spells every field's bin), and ``NormContinuous`` at its knots. The
    interpolation runs in float64 on float64 knots, as in the oracle; each column is then rounded to
    fp32 once (tests/test_gpu_derive.py pins the columns bit for bit) and the regression behind it
    sums in fp32: a score of up to 64 + 256 * 64 carries half an fp32 ulp, 2**13 * 2**-24 < 5e-4, plus
    the two column roundings times their coefficients, against jumps of 63 (or 63 * 256) when an
    input falls on the wrong side of an outer knot — so 1e-3 separates the two."""
    from flink_jpmml_amd.runtime.derive import DerivedPlan

    X = _derive_inputs()
    c = CompiledPmml.from_string(discretize_doc(dtype))
    plan = c.plan(gpu)
    assert isinstance(plan, DerivedPlan)
    ref, vref = c.score_matrix_oracle(X.astype(np.float64))
    B.assert_fp32_exact(ref, vref)
    s, v = _score(plan, X)
    _assert_same(s, v, ref, vref, f"Discretize {dtype}")
    c = CompiledPmml.from_string(norm_doc(dtype))
    plan = c.plan(gpu)
    assert isinstance(plan, DerivedPlan)
    ref, vref = c.score_matrix_oracle(X.astype(np.float64))
    s, v = _score(plan, X)
    assert np.array_equal(v, vref)
    err = np.abs(s[vref].astype(np.float64) - ref[vref])
    print(f"NormContinuous {dtype}: max |device - oracle| = {err.max()!r}")
    assert err.max() <= 1e-3


# --------------------------------------------------------------------------- segment predicates

SEG_OPS = ["equal", "notEqual", "lessThan", "lessOrEqual", "greaterThan", "greaterOrEqual"]
SEG_CONSTS = [0.75, 0.3, 0.7]  # fp32-exact, rounds up in fp32, rounds down in fp32


def segment_doc(dtype: str) -> str:
    """``multipleModelMethod="sum"`` over 18 segments, one per (operator, constant), each a
    one-leaf tree scoring 2**i on field ``f(i % 3)``: the sum names the segments whose predicate
    held."""
    dd = "".join(f'<DataField name="f{j}" optype="continuous" dataType="{dtype}"/>' for j in range(3))
    dd += '<DataField name="y" optype="continuous" dataType="double"/>'
    ms = '<MiningSchema><MiningField name="y" usageType="target"/>' + "".join(
        f'<MiningField name="f{j}"/>' for j in range(3)) + '</MiningSchema>'
    segs = []
    for i, (op, cst) in enumerate((o, k) for o in SEG_OPS for k in SEG_CONSTS):
        segs.append(f'<Segment id="{i + 1}"><SimplePredicate field="f{i % 3}" operator="{op}" value="{cst}"/>'
                    f'<TreeModel functionName="regression">{ms}<Node id="1" score="{2 ** i}"><True/></Node>'
                    '</TreeModel></Segment>')
    return (f'<PMML version="4.4" xmlns="{NS}"><DataDictionary>{dd}</DataDictionary><MiningModel '
            f'functionName="regression">{ms}<Segmentation multipleModelMethod="sum">{"".join(segs)}</Segmentation>'
            '</MiningModel></PMML>')


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_segment_predicates_on_their_constants(gpu, dtype):
    """``segment.hip::seg_predicate``: all six comparison operators against an fp32-exact and two
    decimal constants, inputs at the constants +-2 ulps and the special values. The score is the
    exact sum of 2**i over the segments that fired (< 2**18), so it is compared bit for bit."""
    c = CompiledPmml.from_string(segment_doc(dtype))
    X = B.boundary_matrix([SEG_CONSTS] * 3, ROWS, 8)
    ref, vref = c.score_matrix_oracle(X.astype(np.float64))
    B.assert_fp32_exact(ref, vref)
    plan = c.plan(gpu)
    assert type(plan).__name__ == "SegmentedPlan"
    s, v = _score(plan, X)
    _assert_same(s, v, ref, vref, f"segment predicates {dtype}")


# --------------------------------------------------------------------------- per-record path


@pytest.mark.gpu
def test_per_record_double_inputs_round_to_nearest_fp32(gpu):
    """``score_row``: a double the record carries (0.8 on a ``double`` field under ``lessOrEqual
    0.8``) is rounded to the nearest fp32, then compared exactly — the result is the oracle's on
    ``float32(x)`` for every record (the deviation docs/PARITY.md lists)."""
    from flink_jpmml_amd import DenseVector
    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.config import ScoringConfig

    txt = gbdt_pmml(n_trees=N_TREES, depth=5, n_features=8, seed=13)
    txt = B.rewrite_thresholds(txt, lambda t: f"{t:.1f}")
    txt = B.integer_leaves(B.set_data_type(B.swap_operator_pair(txt), "double"))
    c = CompiledPmml.from_string(txt)
    cuts = B.split_cuts(txt, 8)
    assert any(0.8 in cu for cu in cuts)
    rng = np.random.default_rng(0)
    X = np.stack([rng.choice(np.asarray(cu), 64) for cu in cuts], axis=1)
    X[0] = 0.8  # the probe: fp32(0.8) > 0.8, so `x <= 0.8` holds for the double and not for the record
    ref32, v32 = c.score_matrix_oracle(X.astype(F32))
    B.assert_fp32_exact(ref32, v32)
    assert v32.all()
    m = PmmlModel.from_string(txt).bind(gpu, ScoringConfig(device=gpu, fallback="error"))
    assert m.on_device
    got = np.array([m.predict(DenseVector(r)).value.get_or_else(float("nan")) for r in X])
    assert np.array_equal(got.astype(F32), ref32.astype(F32))
    s, v = _score(c.plan(gpu), X)  # the batch path rounds the same way
    _assert_same(s, v, ref32, v32, "double inputs, batch")
