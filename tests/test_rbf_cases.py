"""The RBF probes of ``tests/_rbf_cases.py`` are exact, sensitive and honestly bounded (CPU).

For every shape that ``tests/test_gpu_rbf_exact.py`` and ``tests/test_gpu_rbf_bound.py`` run on the
device, with plans lowered under ``lowering_dry_run()``: the exactness guard holds; the closed-form
integers, the dense float64 reference and the float64 oracle agree in every bit after rounding to
fp32; every unit owns a row and every output weight shows; the fp32 twin of the device formula, over
the plan's packed panels un-packed with rbf.hip's own index maps, returns the same bits (this pins
``pack_rbf_panels`` without a GPU) and every named mutant of the panels leaves the rule of its probe.
For the smooth probes the twin stays under the recorded ratios that fix the device's bound."""

import functools

import numpy as np
import pytest

import _exact as E
import _rbf_cases as R
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.nn_plans import RbfPlan
from flink_jpmml_amd.runtime.plans import lowering_dry_run

F32 = np.float32


def _plan(c) -> RbfPlan:
    with lowering_dry_run():
        plan = c.plan("cpu")
    assert type(plan) is RbfPlan
    return plan


_same = R.same_bits


def _same64(ref64, want) -> bool:
    """A float64 result against the expected fp32 bits. Where the exact value is 0 the float64 sum
    keeps the units' 1e-56 terms, which round to a zero of either sign: the sign of zero is dropped
    on that side (the twin and the device are compared with it)."""
    return _same(np.asarray(ref64, F32) + F32(0.0), want)


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


EXACT = [(n_in, H, n_out, hn, False) for n_in, H, n_out in R.EXACT_SHAPES for hn in R.HIDDEN_NORMS] + R.CENTROID_CASES


@functools.lru_cache(maxsize=None)
def _exact_case(n_in, H, n_out, hn, centroid=False, missing=False):
    kw = dict(centroid=R.nonzero_centroid(n_in)) if centroid else {}
    p = R.exact_probe(n_in, H, n_out, hn, missing=missing, **kw)
    return p, CompiledPmml.from_string(p.pmml())


@pytest.mark.parametrize("n_in,H,n_out,hn,shifted", EXACT, ids=_ids(EXACT))
def test_onehot_probe_is_exact_and_shows_every_weight(n_in, H, n_out, hn, shifted):
    p, c = _exact_case(n_in, H, n_out, hn, shifted, shifted)
    R.onehot_guard(p)
    assert np.array_equal(p.mu, R.nonzero_centroid(n_in) if shifted else np.zeros(n_in))
    want, ref = R.onehot_expected(p), p.reference()
    # the expected values are integers, or halves over a duplicated centre under simplemax
    E.assert_exact([want["z"]], dyadic=0.5 if hn else 1.0)
    assert hn or np.array_equal(want["z"][want["valid"]], np.round(want["z"][want["valid"]]))
    # closed form = dense float64 reference = oracle, in every fp32 bit
    so, vo = c.score_matrix_oracle(p.fields())
    assert np.array_equal(vo, want["valid"]) and np.array_equal(ref["valid"], vo)
    # classes tied at a largest logit of exactly 0: float64 orders them by the other units' 1e-56 terms
    # (either way); the exact answer, the first of them, is what the device is held to
    with np.errstate(invalid="ignore"):
        zero_tie = ((want["out"] == 0) & (np.nanmax(want["out"], axis=1, keepdims=True) == 0)).sum(axis=1) > 1
    assert zero_tie.mean() < 0.1
    assert _same64(ref["score"][~zero_tie], want["score"][~zero_tie]) and _same64(so[~zero_tie], want["score"][~zero_tie])
    assert _same64(ref["out"], want["out"]) and not np.signbit(want["out"][want["out"] == 0]).any()
    if p.classification:
        assert _same64(c.result(p.fields()).probs, want["out"])
    # every unit owns a valid row on its centre (also within the first 257 rows for the small shapes):
    # a changed V[k, j] then changes output k of that row
    owned = set(p.unit[want["valid"] & (p.unit >= 0)].tolist())
    assert owned == set(p.head.tolist())
    assert len(p.Xi) >= 264 and np.isnan(p.Xi[list(R.NAN_POSITIONS)]).any(axis=1).all()
    assert not want["valid"][list(R.NAN_POSITIONS)].any()
    if hn is None:  # a row no unit fires on gives the bias alone
        assert (want["valid"] & (p.unit < 0)).any()
    if p.classification and n_out > 5:  # exact ties between classes 4 apart: the first maximum wins
        top = want["out"] == np.nanmax(want["out"], axis=1, keepdims=True)
        assert (want["valid"] & top[:, 1] & top[:, 5]).any()
    if shifted:  # the replaced row is valid and equals its twin
        nan_row = np.flatnonzero(np.isnan(p.Xi[:, 0]) & np.isnan(p.Xi[:, -1]) & ~np.isnan(p.Xi[:, 1]))[0]
        assert want["valid"][nan_row] and _same(want["out"][nan_row], want["out"][nan_row + 1])
    # the twin over the packed panels: the packer's layout is what rbf.hip's index maps read
    plan = _plan(c)
    got = R.twin_outputs(p, R.twin(plan, p.fields()))
    assert np.array_equal(got["valid"], want["valid"]) and _same(got["out"], want["out"])
    assert _same(got["score"], want["score"])


def test_routes_of_the_input_stage_lower_as_intended():
    """Identity order is the vector path, a permutation or a leading unread field the gather path;
    unread trailing fields keep the vector path with a longer row."""
    for n_in, H, n_out in R.ROUTE_SHAPES:
        p = R.exact_probe(n_in, H, n_out, None)
        want = R.onehot_expected(p)
        perm = R.permutation(n_in + 3)[:n_in]
        for order, extra, contiguous in ((None, 0, 1), (R.permutation(n_in), 0, 0), (None, 3, 1), (perm, 3, 0)):
            c = CompiledPmml.from_string(p.pmml(order, extra))
            plan = _plan(c)
            assert plan.contiguous == contiguous and c.n_features == n_in + extra
            X = p.fields(order, extra)
            so, vo = c.score_matrix_oracle(X)
            assert np.array_equal(vo, want["valid"]) and _same64(so, want["score"])
            got = R.twin_outputs(p, R.twin(plan, X))
            assert _same(got["out"], want["out"]) and np.array_equal(got["valid"], want["valid"])


@pytest.mark.parametrize("act", R.A.ACTS)
def test_output_activation_probe(act):
    """Pre-activations of the activation probe are exact, ``threshold`` has rows exactly on it and the
    oracle equals ``activate`` on them."""
    p = R.activation_probe(act)
    want = R.onehot_expected(p)
    z = want["z"][want["valid"]]
    E.assert_exact([z], dyadic=1.0 / 32)
    assert np.abs(z).max() <= R.A.DOMAIN[act]
    if act == "threshold":
        assert (z == p.out_thr).any() and (z > p.out_thr).any() and (z < p.out_thr).any()
    if act == "reciprocal":
        assert (z != 0).all()
    c = CompiledPmml.from_string(p.pmml())
    so, vo = c.score_matrix_oracle(p.fields())
    assert np.array_equal(vo, want["valid"]) and _same64(so, want["score"])
    assert _same64(c.result(p.fields()).probs, want["out"])


def test_target_stage_probe():
    """Rescale by 2, constant -1, ``castInteger="round"`` on the one-hot regression: 2 z - 1 exactly."""
    p = R.target_probe()
    want = R.onehot_expected(p)
    so, vo = CompiledPmml.from_string(p.pmml()).score_matrix_oracle(p.fields())
    assert np.array_equal(vo, want["valid"]) and _same64(so, want["score"])
    assert np.array_equal(want["score"][vo], 2.0 * want["z"][vo, 0] - 1.0)


@pytest.mark.parametrize("n_in,H,n_out", R.MUTANT_SHAPES, ids=_ids(R.MUTANT_SHAPES))
def test_every_panel_mutant_shows(n_in, H, n_out):
    """On the twin: every mutant but the c / g swaps changes a compared bit of a one-hot probe (under
    ``none`` or under ``simplemax``); the c, g and norm swaps leave the bound of a smooth probe."""
    runs = []
    for hn in R.HIDDEN_NORMS:
        p = R.exact_probe(n_in, H, n_out, hn)
        plan = _plan(CompiledPmml.from_string(p.pmml()))
        runs.append((p, plan, R.onehot_expected(p)))
    kp = runs[0][1].kp
    muts = R.panel_mutants(kp, H, n_out)
    if H == 70:
        assert len(muts) == 14 and "padded-unit-finite-norm" in muts and "swap-g-32-apart" in muts
    for name, f in muts.items():
        if name.startswith(R.SMOOTH_ONLY):
            continue
        seen = False
        for p, plan, want in runs:
            pan = plan.panels.numpy().reshape(plan.n_tiles, -1).copy()
            f(pan)
            got = R.twin_outputs(p, R.twin(plan, p.fields(), pan))
            seen |= not (_same(got["out"], want["out"]) and np.array_equal(got["valid"], want["valid"]))
        assert seen, f"mutant {name} changes no compared bit"
    sp = R.smooth_probe(n_in, H, n_out, seed=n_in + H)
    plan = _plan(CompiledPmml.from_string(sp.pmml()))
    ref = sp.reference()
    for name, f in muts.items():
        if not name.startswith(R.SMOOTH_ONLY + ("swap-norm-",)):
            continue
        pan = plan.panels.numpy().reshape(plan.n_tiles, -1).copy()
        f(pan)
        ratio, _ = R.check_bound(sp, ref, R.twin_outputs(sp, R.twin(plan, sp.fields(), pan))["out"])
        assert ratio > R.C, f"mutant {name}: ratio {ratio:.3g} stays under C = {R.C}"


BOUND = R.bound_cases()


@pytest.mark.parametrize("n_in,H,n_out,hn,fn", BOUND, ids=_ids(BOUND))
def test_twin_stays_under_the_bound(n_in, H, n_out, hn, fn):
    """The fp32 twin against the float64 closed form (itself equal to the oracle): its ratio is what
    ``_rbf_cases.TWIN_RATIO`` records, and the reference alone leaves at most 2 % of the rows unclear."""
    p = R.bound_probe(n_in, H, n_out, hn, fn)
    c = CompiledPmml.from_string(p.pmml())
    ref = p.reference()
    so, vo = c.score_matrix_oracle(p.fields())
    assert np.array_equal(vo, ref["valid"]) and not vo[7] and not vo[11] and vo.sum() == len(vo) - 2
    if p.classification:
        Po = c.result(p.fields()).probs
        scale = ref["T"] if fn is None else 1.0
        assert (np.abs(Po - ref["out"])[vo] <= 1e-12 * (scale[vo] if fn is None else 1.0)).all()
        assert np.array_equal(so[vo], ref["score"][vo])
    else:
        assert (np.abs(so - ref["score"])[vo] <= 1e-12 * ref["T"][vo, 0]).all()
    a, _, g, d = p.hidden(p.inputs()[0])
    assert 0.05 < np.median(a.max(axis=1)) <= 1.1  # activations of order 0.1 to 1, none underflows
    assert a.min() > 1e-30
    got = R.twin_outputs(p, R.twin(_plan(c), p.fields()))
    ratio, tol = R.check_bound(p, ref, got["out"])
    left = 1.0 - R.clear_rows(p, ref, tol)[vo].mean() if p.classification else 0.0
    print(f"RBF_TWIN_RATIO {n_in}-{H}-{n_out} {hn} {fn}: {ratio:.4f}, {left:.2%} of the rows left out")
    assert np.array_equal(got["valid"], ref["valid"])
    assert ratio <= R.TWIN_RATIO[f"{n_in}-{H}-{n_out}"]
    assert left <= 0.02
