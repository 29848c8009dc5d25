"""CPU half of the wide-kernel probes (tests/_wide_cases.py): every case lowers as named and reaches
what it exists for (computed from the plan), the oracle's results pass the exactness guard, the
numpy twin of the kernel equals the oracle on both blobs, and the named mutants of a packed plan
change a compared bit. GPU half: tests/test_gpu_wide_cases.py."""

import numpy as np
import pytest

from tests import _boundary as B
from tests import _epilogue_cases as E
from tests import _wide_cases as W

from flink_jpmml_amd.runtime.plans import TreePlan

NAMES = [c.name for c in W.CASES]


def _paths(plan, X):
    """(use_nan_blob, rows that path can see): with a NaN blob the main blob only ever walks tiles
    without missing values."""
    stage = plan.feat_map.numpy() if plan.feat_map is not None else np.arange(X.shape[1])
    clean = ~np.isnan(X[:, stage]).any(axis=1)
    if plan.blob_nan is None:
        return [(False, np.ones(len(X), bool))]
    return [(False, clean), (True, np.ones(len(X), bool))]


def _twin_differs(plan, X, ref, vref, **kw) -> bool:
    for use_nan, keep in _paths(plan, X):
        try:
            out = W.emulate_wide(plan, X[keep], use_nan, **kw)
        except AssertionError:
            return True
        r, v = ref[keep], vref[keep]
        if not np.array_equal(np.isfinite(out), v) or not np.array_equal(out[v], r[v]):
            return True
    return False


@pytest.mark.parametrize("name", NAMES)
def test_case_lowers_as_named_and_twin_equals_oracle(name):
    case = W.CASE[name]
    plan = W.dry_plan(case)
    W.assert_lowering(case, plan)
    X, Y, (ref, vref), (refy, vrefy) = W.reference(case.doc, case.rows)
    assert vref.any() and (case.nan != "off" or "null" not in case.doc or not vref.all())
    if plan.mode == 0:
        B.assert_fp32_exact(ref, vref)  # integer leaves (+ 0.5): exact in fp32 in any order
        B.assert_fp32_exact(refy, vrefy)
    elif plan.mode == 1:
        # integer leaves -2..2 and intercepts 1..3: every class logit is an integer far below 2**24
        _, _, po = E.oracle(W.doc(case.doc).compiled, X)
        logit = np.log(po[vref])
        d = logit - logit[:, :1]  # logit differences of a softmax: integers when the logits are
        assert np.abs(d - np.round(d)).max() < 1e-9 and np.abs(d).max() < 2 ** 10
        leaves = np.array([t.leaf_value[t.feature < 0] for t in plan.spec.trees]).ravel()
        assert np.array_equal(leaves, np.round(leaves)) and np.abs(leaves).max() <= 2
        assert np.array_equal(plan.acc_init.numpy(), np.round(plan.acc_init.numpy()))
    elif plan.mode == 2 and plan.tree_w is not None:
        w = plan.tree_w.numpy().astype(np.float64)
        assert np.isin(w, (0.5, 1, 2, 4)).all() and w.sum() < 2 ** 23  # dyadic vote totals
    for M, r, v in ((X, ref, vref), (Y, refy, vrefy)):
        for use_nan, keep in _paths(plan, M):
            out = W.emulate_wide(plan, M[keep], use_nan)
            if case.doc == "fmap300":  # the twin walks trees only: the interval's verdict by construction
                x = M[:, W.FMAP_PREP].astype(np.float64)
                outside = ~np.isnan(x) & ~((x >= -1.0) & (x < 1.0))
                assert np.array_equal(v, ~outside) and outside.any() and not outside.all()
                out = np.where(outside[keep], np.nan, out)
            assert np.array_equal(np.isfinite(out), v[keep]), (name, use_nan)
            assert np.array_equal(out[v[keep]], r[keep][v[keep]]), (name, use_nan)
    # the forced matrix: a clean first tile, one missing value in the second
    stage = plan.feat_map.numpy() if plan.feat_map is not None else np.arange(Y.shape[1])
    miss = np.isnan(Y[:, stage]).any(axis=1)
    assert not miss[:case.rows].any() and miss[case.rows:].sum() == 1


def test_static_groups_walk_every_tail_width():
    """Over the 128- and 64-row SUM cases a group's tree count takes every value 1..15: every
    8 / 4 / 2 / 1 combination of ``traverse_fast_g``'s batches."""
    mt = set()
    for name in W.STATIC_SUM_CASES:
        case = W.CASE[name]
        assert case.launch == dict(splits=1)  # one slice: the groups walk whole chunks
        mt |= W.case_coverage(case, W.dry_plan(case))["mt"]
    assert mt >= set(range(1, 16)), sorted(mt)


def test_dynamic_batches_end_on_every_remainder():
    tails = set()
    for n in (1, 7, 8, 9, 12, 14, 15, 17):
        tails |= W.case_coverage(W.CASE[f"sum{n}"], W.dry_plan(W.CASE[f"sum{n}"]))["tail"]
    assert tails == {0, 1, 4, 6, 7}  # 7 = 4 + 2 + 1, 6 = 4 + 2: each of the 4 / 2 / 1 branches taken and skipped


def test_splits_leave_an_empty_slice():
    """``launch(splits=4)`` of one tree: trees_per_split = 1 and the launcher drops the empty slices;
    19 trees: 5 + 5 + 5 + 4."""
    for name, chunks in (("sum1-splits4", 1), ("sum19-splits4", 4)):
        assert W.CASE[name].launch == dict(splits=4)
        assert W.case_coverage(W.CASE[name], W.dry_plan(W.CASE[name]))["chunks"] == chunks


@pytest.mark.parametrize("mutant", list(W.PLAN_MUTANTS))
def test_every_named_mutant_changes_a_compared_bit(mutant):
    applies, mutate, kw = W.PLAN_MUTANTS[mutant]
    tripped = []
    for case in W.CASES:
        if case.doc.startswith(("cap", "sum367", "sum183", "sum131")) and case.name != "cap640-c5":
            continue  # the large forests add nothing here
        plan = W.dry_plan(case)
        if not applies(plan):
            continue
        X, _, (ref, vref), _ = W.reference(case.doc, case.rows)
        if _twin_differs(mutate(plan), X, ref, vref, **kw):
            tripped.append(case.name)
    assert tripped, mutant
    print(f"{mutant}: {len(tripped)} cases")


# ------------------------------------------------------------------ the VOTE8 counter bound


@pytest.mark.parametrize("name", [c.name for c in W.CASES if c.doc.startswith("cap")])
def test_unanimous_rows_vote_their_class(name):
    """Row k of ``UNANIMOUS_ROWS`` reaches leaf position k of every tree: the oracle's label is
    that position's class, whatever the plan; the split-vote row stays with class 0."""
    case = W.CASE[name]
    d = W.doc(case.doc)
    _, _, (ref, vref), _ = W.reference(case.doc, case.rows)
    C = {"cap1020": 4, "cap640": 3, "cap1000": 4, "cap640-split": 2, "cap900": 4}[d.name]
    for k, r in enumerate(W.UNANIMOUS_ROWS):
        assert vref[r]
        if k == 0 and case.doc == "cap640-split":
            assert ref[r] == 0.0  # 256 + 190 votes of 640
        else:
            assert ref[r] == float(k % C), (name, k, ref[r])


def test_vote8_only_where_no_counter_can_pass_255():
    """The kernel gives group g the trees ``k = g (mod G)`` of *every* chunk. A chunk of 5 (7)
    trees at G = 4 hands group 0 two trees a chunk: 256 of 640 (286 of 1000). The lowering rounds
    VOTE8 chunks to multiples of G, and falls back to MODE_CLASS where that is not enough."""
    peak = TreePlan.vote8_peak
    assert peak(640, 5, 4) == 256 and peak(1000, 7, 4) == 286 and peak(300, 7, 4) == 86  # the old chunks
    # depth 10 chunked 7 trees on its own (no forest that large is lowered here: the count alone)
    assert peak(893, 7, 4) == 255 and peak(894, 7, 4) == 256 and peak(894, 4, 4) == 224
    assert peak(1020, 64, 4) == 255 and peak(640, 4, 4) == 160 and peak(1000, 4, 4) == 250
    for name, mode, chunk in (("cap1020", 3, 64), ("cap640-c5", 3, 4), ("cap1000-c7", 3, 4), ("cap900-c3", 2, 3)):
        plan = W.dry_plan(W.CASE[name])
        assert (plan.mode, plan.chunk_trees, plan.chunk_trees_nan) == (mode, chunk, chunk), name
        assert plan.mode != 3 or W.peak(plan) <= 255
    plan = W.dry_plan(W.CASE["vote9-d10"])  # the natural shape: 7 depth-10 records fit a chunk buffer
    assert plan.depth == 10 and plan.n_trees == 9 and plan.chunk_trees == 4 == plan.chunk_trees_nan  # 7 before
