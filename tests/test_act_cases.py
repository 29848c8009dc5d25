"""The activation and normalisation probes of ``tests/_act_cases.py`` are exact and sensitive (CPU).

For every (kernel path, site, activation) that ``tests/test_gpu_activations.py`` runs on the
device: the float64 oracle's score on the document equals ``models.neural.activate`` on the
closed-form pre-activations in every bit, the exactness guards hold, the batch covers the stated
domain and hits its special points, no unit that the outputs do not read sits on a pole, and every
named mutant of the device formulas leaves the comparison rule with the committed constants — a
mutant that stays inside a bound means the bound (or the domain) is too wide, not that the kernel
is right."""

import numpy as np
import pytest
import torch

import _act_cases as A
import _exact as E
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.nn_plans import MlpPlan, WideMlpPlan, pad_bias
from flink_jpmml_amd.runtime.plans import compile_plan, lowering_dry_run


def _plan(c, **kw):
    with lowering_dry_run():
        return compile_plan(c, torch.device("cpu"), **kw)


def _oracle(c, ramp, X):
    """The oracle's ``(outputs [rows, n_out], valid)`` of a ramp document."""
    if ramp.classification:
        r = c.result(X)
        return r.probs, r.valid
    s, v = c.score_matrix_oracle(X)
    return s[:, None], v


def test_default_documents_are_unchanged():
    """``nn_pmml`` without the new arguments writes what it wrote before: rectifier hidden layers, an
    identity output layer, no threshold and no network-level normalisation."""
    layers = E.int_network(5, (6,), 3, seed=1)
    doc = E.nn_pmml(layers, True, "softmax")
    assert doc.count('<NeuralLayer>') == 1 and doc.count('threshold=') == 0
    assert '<NeuralNetwork functionName="classification" activationFunction="rectifier">' in doc
    assert '<NeuralLayer activationFunction="identity" normalizationMethod="softmax">' in doc


@pytest.mark.parametrize("name,tested", A.SITES)
def test_oracle_equals_reference_and_plans_lower(name, tested):
    """Oracle = float64 ``activate`` on the exact z, outputs and validity, for all 13 activations
    (threshold on the layer and on the network) and both seeds; the document lowers to the plan class
    of its path in both precisions; no unread unit holds a non-finite or fp32-overflowing value."""
    cls = MlpPlan if name in A.FUSED_PATHS else WideMlpPlan
    for variant in A.VARIANTS:
        for seed in A.SEEDS:
            r = A.ramp(name, tested, variant, seed)
            X = A.ramp_matrix(A.ROWS, r.n_in, seed)
            ref, valid, z = r.reference(X)  # asserts the exactness guards
            assert np.abs(z).max() <= A.DOMAIN[r.act], variant[0]
            assert r.unread_poles(X) == 0, variant[0]
            c = CompiledPmml.from_string(r.pmml())
            out, v = _oracle(c, r, X)
            fin = valid & np.isfinite(ref).all(axis=1)
            assert np.array_equal(v, valid if r.classification else fin), variant[0]
            assert np.array_equal(out[fin], ref[fin]), variant[0]
            if seed == 0:
                for precision in ("fp32", "bf16"):
                    plan = _plan(c, precision=precision)
                    assert type(plan) is cls, (variant[0], precision, type(plan))
                    thr = plan.layer_meta.numpy()[tested, 6:7].view(np.float32)[0] if cls is MlpPlan \
                        else plan.dims[tested][3]
                    assert thr == r.thr, variant[0]


@pytest.mark.parametrize("name,tested", A.SITES)
def test_batch_covers_the_domain(name, tested):
    """Over the two seeds, the z of the compared entries (valid rows) hit 0, +-thr and the ends +-16
    exactly, leave no gap wider than 1/4 in [-16, 16] and none wider than 1/16 in [-4, 4]; -0.0 is
    among the input cells the tested units read (the input stage's fused multiply-add and the bias
    add turn it into +0.0 on the device and in the oracle alike: no pre-activation is ever -0.0)."""
    zs, neg_zero = [], False
    for seed in A.SEEDS:
        r = A.ramp(name, tested, A.VARIANTS[0], seed)
        X = A.ramp_matrix(A.ROWS, r.n_in, seed)
        _, valid, z = r.reference(X)
        zs.append(z[valid].ravel())
        neg_zero = neg_zero or bool(np.signbit(X[valid][X[valid] == 0]).any())
        assert not np.signbit(z[z == 0]).any()
    z = np.unique(np.concatenate(zs))
    for point in (0.0, A.THR, -A.THR, 16.0, -16.0):
        assert point in z, point
    assert neg_zero
    assert np.diff(z).max() <= 0.25 and np.diff(z[np.abs(z) <= 4]).max() <= 1.0 / 16


def _mutant_checks(r, X, mutants):
    for bf16_hidden in ((False, True) if r.tested < len(r.sizes) - 1 else (False,)):
        want, tol, ref, valid, z = A.expected(r, X, bf16_hidden)
        valid = valid & np.isfinite(ref).all(axis=1)
        z32 = z.astype(np.float32)
        assert np.array_equal(z32.astype(np.float64), z)

        def device(f):
            with np.errstate(all="ignore"):
                v = f(z32, r.thr)
                if r.tested < len(r.sizes) - 1 and r.post_act != "identity":
                    v = A.twin_activate(r.post_act, v)
            return A.bf16_rn(v) if bf16_hidden else v

        assert not A.caught(device(lambda zz, t: A.twin_activate(r.act, zz, t)), want, tol, ref, valid), \
            f"{r.act}: the unmutated twin fails its own rule (bf16 {bf16_hidden})"
        for mname, f in mutants.items():
            assert A.caught(device(f), want, tol, ref, valid), f"{mname} (seed {r.seed}, bf16 {bf16_hidden}) not caught"


@pytest.mark.parametrize("name,tested", A.SITES)
def test_every_activation_mutant_is_caught(name, tested):
    """Each activation code replaced by each other one, ``>=`` for ``>``, the network's threshold for
    the layer's, arctan without 2/pi, Gauss with +z^2, logistic without the negation, sine for
    cosine, padded units left at reciprocal(0): all leave the rule (bits, or the bound with the
    committed constants) on at least one compared entry, with either seed, in fp32 and in bf16."""
    for variant in A.VARIANTS:
        for seed in A.SEEDS:
            r = A.ramp(name, tested, variant, seed)
            X = A.ramp_matrix(A.ROWS, r.n_in, seed)
            _mutant_checks(r, X, A.activation_mutants(r.act, r.layer_thr is not None))


@pytest.mark.parametrize("name", A.TWO_SITE)
def test_swapped_sites_are_caught(name):
    """Rectifier in the hidden layer and square in the output layer: applying each at the other's
    site changes every entry with z < 0."""
    for seed in A.SEEDS:
        r = A.ramp(name, 0, ("rectifier", "rectifier", None, None), seed, post_act="square")
        X = A.ramp_matrix(A.ROWS, r.n_in, seed)
        ref, valid, z = r.reference(X)
        assert np.array_equal(ref, np.maximum(z, 0.0) ** 2)
        c = CompiledPmml.from_string(r.pmml())
        out, v = _oracle(c, r, X)
        assert np.array_equal(v, valid) and np.array_equal(out[valid], ref[valid])
        _mutant_checks(r, X, {"sites swapped": lambda zz, t: np.abs(zz)})  # the output's square follows: z^2 = rectifier(square(z))


def test_padded_units_of_a_reciprocal_layer_are_finite():
    """The padded units of a hidden layer (zero weights) get a bias whose activation is finite: 1 for
    reciprocal, whose value at 0 would meet the next layer's stored zeros as ``0 * inf``."""
    assert pad_bias("reciprocal") == 1.0 and all(pad_bias(a) == 0.0 for a in A.ACTS if a != "reciprocal")
    for name, tested in (("17-33-1", 0), ("33-300-1", 0), ("65-257-300-1", 1)):
        r = A.ramp(name, tested, ("reciprocal", "reciprocal", None, None), 0)
        plan = _plan(CompiledPmml.from_string(r.pmml()), precision="fp32")
        m = r.sizes[tested]
        if isinstance(plan, WideMlpPlan):
            kp, mp, act, thr, wo, bo = plan.dims[tested]
        else:
            kp, mp, mreal, wo, bo, act = (int(v) for v in plan.layer_meta.numpy()[tested, :6])
        b = (plan.bss if isinstance(plan, WideMlpPlan) else plan.biases).numpy()[bo: bo + mp]
        assert mp > m and (b[m:] == 1.0).all() and np.array_equal(b[:m], r.b.astype(np.float32))


# --------------------------------------------------------------------------- row normalisation


@pytest.mark.filterwarnings("ignore:.*encountered in divide")  # the oracle on the zero-sum rows
@pytest.mark.parametrize("name", list(A.NORM_FUSED) + list(A.NORM_WIDE))
def test_normalisation_probe_is_exact_and_sensitive(name):
    """Logits k/4 with |k| <= 64 and exact sums; the oracle's probabilities equal ``normalize_layer`` on
    them; rows with a negative, a power-of-two and a zero logit sum and rows whose maximum is tied
    are present; the fp32 twin keeps the rule (simplemax: bit for bit; softmax: the bound) and each
    mutant (padded units in the sum, one lane half's sum, simplemax over |z|, last of ties) leaves it."""
    n_in, hidden, n_out = {**A.NORM_FUSED, **A.NORM_WIDE}[name]
    net = A.Logits(n_in, hidden, n_out)
    X = net.matrix(A.ROWS)
    Z, valid = net.logits(X)
    sums = Z.sum(axis=1)
    assert valid[0] and sums[0] == 0 and Z[0].any()
    pos = sums[valid & (sums > 0)]
    assert (sums[valid] < 0).any() and (np.frexp(pos)[0] == 0.5).any()
    if n_out >= 4:
        assert np.array_equal(Z[:, -1], Z[:, net.dup]) and (Z[valid].argmax(axis=1) == net.dup).any()
    cls = MlpPlan if name in A.NORM_FUSED else WideMlpPlan
    for norm in A.NORMS:
        c = CompiledPmml.from_string(net.pmml(norm))
        for precision in ("fp32", "bf16"):
            plan = _plan(c, precision=precision)
            assert type(plan) is cls and plan.final_norm == {"softmax": 1, "simplemax": 2, None: 0}[norm]
        P, label, S = A.norm_reference(Z, norm)
        ok = valid & (sums != 0) if norm == "simplemax" else valid
        res = c.result(X)
        assert np.array_equal(res.valid, valid) and np.array_equal(res.probs[ok], P[ok])
        so, vo = c.score_matrix_oracle(X)
        assert np.array_equal(vo, valid) and np.array_equal(so[ok], label[ok].astype(np.float64))

        def rule_broken(p, lab):
            if not np.array_equal(lab[ok], label[ok]):
                return True
            if norm == "softmax":
                return bool((~(np.abs(p[ok].astype(np.float64) - P[ok]) <= A.SOFTMAX_C * A.U * S[ok])).any())
            return not np.array_equal(E.bits(p[ok]), E.bits(P[ok].astype(np.float32)))

        assert not rule_broken(*A.twin_normalize(Z, norm)), norm
        for m in A.norm_mutants(norm, n_out):
            assert rule_broken(*A.twin_normalize(Z, norm, m)), (norm, m)


@pytest.mark.filterwarnings("ignore:.*encountered in divide")  # the oracle on the zero-sum rows
def test_network_level_normalisation_reaches_the_output_layer():
    """``normalizationMethod`` on the NeuralNetwork element is inherited by every layer, so it lowers
    only for a network of one layer (hidden-layer normalisation is host-only); there the plan and
    the oracle take it as the output layer's."""
    net = A.Logits(12, (), 7)
    c = CompiledPmml.from_string(net.pmml(None, net_normalization="simplemax"))
    assert _plan(c, precision="fp32").final_norm == 2
    X = net.matrix(33)
    Z, valid = net.logits(X)
    P, _, _ = A.norm_reference(Z, "simplemax")
    ok = valid & (Z.sum(axis=1) != 0)
    assert np.array_equal(c.result(X).probs[ok], P[ok])
