"""Probes for the radial-basis-function network kernel (rbf.hip), in the style of ``tests/_exact.py``.

Two kinds of network, both with caller-chosen parameters (``bench/synth.py`` only draws random ones,
always with an identity output layer, inputs in field order and no missing replacement):

* the *one-hot* probe: distinct small-integer centres, every width 1/16 (``g = 128``), altitude 1
  (``c = 0``), integer output weights. A row on a centre has ``d = 0`` for that unit and ``g d >= 128``
  for every other one, which fp32 ``exp`` returns 0 for and float64 at most 2.6e-56: the outputs are
  the integers ``V[:, j] + b`` (summed, or under ``simplemax`` averaged, over a duplicated centre) in
  every bit, so a wrong panel entry, permutation, mask, tail or tie is a whole-integer difference;
* the *smooth* probe: integer centres and inputs, widths near ``2 sqrt(n_in)``, activations of order
  0.01 to 1. The kernel is held to ``C 2^-24 T`` of the dense float64 closed form, with ``T`` the
  magnitude an fp32 evaluation's rounding errors scale with and ``C`` set from an fp32 numpy twin of
  the device formula, measured on the CPU against the float64 reference (never against the kernel).

This module holds the document builder, the probes with their inputs and references, the un-packer
of ``pack_rbf_panels`` (written from rbf.hip's index maps, not from the packer), the twin and the
named mutants of the packed panels."""

import io
from typing import Dict, Optional, Sequence

import numpy as np

import _act_cases as A
import _exact as E
from flink_jpmml_amd.bench.synth import _data_dictionary, _header, _mining_schema
from flink_jpmml_amd.models.neural import activate, normalize_layer

F32 = np.float32
U = 2.0 ** -24
TAIL = 1024 + 128  # panel floats after the centre fragments (rbf.hip)
FILL = 97.0  # what an unread column holds (``_exact.strided`` uses the same)
NAN_POSITIONS = (0, 31, 32, 63, 64, 255, 256)  # rows with one NaN: the tile, wave and workgroup seams
ROW_COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
HUGE = 3e19  # its square overflows fp32

# ---- the fp32 twin (``twin``) against the float64 reference on the cases of BOUND_CASES, measured
# on the CPU by tests/test_rbf_cases.py::test_twin_stays_under_the_bound: the largest
# |twin - reference| / (2^-24 T) per shape, over every hidden / final normalisation. C is 4 x the
# largest, the margin SVM_ULP_CONSTANT and _act_cases.C use: room for the MFMA summation order and __expf.
TWIN_RATIO = {"3-33-1": 0.83, "17-70-5": 0.62, "40-96-3": 0.55, "8-1024-3": 0.57, "128-33-2": 0.62}
C = 4.0 * max(TWIN_RATIO.values())  # 3.32


def same_bits(a, b) -> bool:
    """Equal fp32 bit patterns, a NaN equal to any NaN (0 / 0 and ``np.nan`` differ in the sign bit)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and np.array_equal(E.bits(a)[~na], E.bits(b)[~na])


def _num(v) -> str:
    v = float(v)
    return str(int(v)) if v == int(v) and abs(v) < 1e15 else repr(v)


# --------------------------------------------------------------------------- the document


def rbf_document(centers: np.ndarray, width: np.ndarray, altitude: np.ndarray, V: np.ndarray, bias: np.ndarray,
                 out_act: str = "identity", out_thr: Optional[float] = None, hidden_norm: Optional[str] = None,
                 final_norm: Optional[str] = None, classification: bool = False,
                 order: Optional[Sequence[int]] = None, extra: int = 0, map_missing: Optional[Dict[int, float]] = None,
                 target: Optional[dict] = None) -> str:
    """RBF NeuralNetwork: ``centers [H, n_in]`` (NeuralInput order), per-unit ``width`` / ``altitude``
    written on every Neuron, output weights ``V [n_out, H]`` and ``bias``. NeuralInput i reads DataField
    ``f{order[i]}`` of ``n_in + extra`` fields (the ``extra`` last ones are MiningFields no input reads)
    through the identity LinearNorm of ``_exact.nn_pmml`` (``in_scale = 1``, ``in_shift = 0``), with
    ``mapMissingTo`` on the inputs of ``map_missing``. ``target``: ``dict(factor, constant, cast)``."""
    H, n_in = centers.shape
    n_out = V.shape[0]
    order = list(range(n_in)) if order is None else [int(o) for o in order]
    assert len(set(order)) == n_in and max(order) < n_in + extra
    out = io.StringIO()
    _header(out, f"RBF probe {n_in}-{H}-{n_out}")
    _data_dictionary(out, n_in + extra, "y", "integer" if classification else "double",
                     [str(k) for k in range(n_out)] if classification else None)
    fn = "classification" if classification else "regression"
    out.write(f' <NeuralNetwork functionName="{fn}" activationFunction="radialBasis">\n')
    _mining_schema(out, n_in + extra, "y", "  ")
    if target is not None:
        cast = f' castInteger="{target["cast"]}"' if target.get("cast") else ""
        out.write(f'  <Targets><Target field="y" rescaleFactor="{_num(target.get("factor", 1.0))}" '
                  f'rescaleConstant="{_num(target.get("constant", 0.0))}"{cast}/></Targets>\n')
    out.write('  <NeuralInputs>\n')
    for i in range(n_in):
        mm = f' mapMissingTo="{_num(map_missing[i])}"' if map_missing and i in map_missing else ""
        out.write(f'   <NeuralInput id="i{i}"><DerivedField optype="continuous" dataType="double">'
                  f'<NormContinuous field="f{order[i]}"{mm}><LinearNorm orig="-1" norm="-1"/>'
                  '<LinearNorm orig="1" norm="1"/></NormContinuous></DerivedField></NeuralInput>\n')
    out.write('  </NeuralInputs>\n')
    out.write('  <NeuralLayer' + (f' normalizationMethod="{hidden_norm}"' if hidden_norm else "") + '>\n')
    for j in range(H):
        out.write(f'   <Neuron id="h{j}" width="{_num(width[j])}" altitude="{_num(altitude[j])}">')
        out.write("".join(f'<Con from="i{i}" weight="{_num(centers[j, i])}"/>' for i in range(n_in)))
        out.write('</Neuron>\n')
    out.write('  </NeuralLayer>\n')
    attrs = f' activationFunction="{out_act}"' + (f' threshold="{_num(out_thr)}"' if out_thr is not None else "")
    out.write(f'  <NeuralLayer{attrs} normalizationMethod="{final_norm or "none"}">\n')
    for k in range(n_out):
        out.write(f'   <Neuron id="o{k}" bias="{_num(bias[k])}">')
        out.write("".join(f'<Con from="h{j}" weight="{_num(V[k, j])}"/>' for j in np.flatnonzero(V[k])))
        out.write('</Neuron>\n')
    out.write('  </NeuralLayer>\n  <NeuralOutputs>\n')
    for k in range(n_out):
        ex = f'<NormDiscrete field="y" value="{k}"/>' if classification else '<FieldRef field="y"/>'
        out.write(f'   <NeuralOutput outputNeuron="o{k}"><DerivedField optype="continuous" dataType="double">'
                  f'{ex}</DerivedField></NeuralOutput>\n')
    out.write('  </NeuralOutputs>\n </NeuralNetwork>\n</PMML>\n')
    return out.getvalue()


class Probe:
    """One network with its input rows ``Xi [rows, n_in]`` (fp32, NeuralInput order)."""

    def __init__(self, centers, width, altitude, V, bias, Xi, hidden_norm=None, final_norm=None,
                 classification=False, out_act="identity", out_thr=None, map_missing=None, target=None):
        self.centers, self.width, self.altitude = np.asarray(centers, np.float64), np.asarray(width), np.asarray(altitude)
        self.V, self.bias, self.Xi = np.asarray(V, np.float64), np.asarray(bias, np.float64), np.asarray(Xi, F32)
        self.hidden_norm, self.final_norm, self.classification = hidden_norm, final_norm, classification
        self.out_act, self.out_thr, self.map_missing, self.target = out_act, out_thr, map_missing, target
        self.H, self.n_in = self.centers.shape
        self.n_out = self.V.shape[0]
        self.mu = self.centers.mean(axis=0)  # what RbfPlan folds into the input stage

    def pmml(self, order=None, extra=0) -> str:
        return rbf_document(self.centers, self.width, self.altitude, self.V, self.bias, self.out_act, self.out_thr,
                            self.hidden_norm, self.final_norm, self.classification, order, extra, self.map_missing,
                            self.target)

    def fields(self, order=None, extra=0, Xi=None) -> np.ndarray:
        """The record matrix ``[rows, n_in + extra]`` of ``pmml(order, extra)``: field ``order[i]`` holds
        input i, a field no input reads holds FILL."""
        Xi = self.Xi if Xi is None else Xi
        order = list(range(self.n_in)) if order is None else list(order)
        X = np.full((len(Xi), self.n_in + extra), FILL, F32)
        X[:, order] = Xi
        return X

    # ---- the dense float64 closed form
    def inputs(self, Xi=None):
        """``(x float64 with the replacements in and NaN as 0, valid)`` of the input stage."""
        X = np.array(self.Xi if Xi is None else Xi, np.float64)
        for i, v in (self.map_missing or {}).items():
            X[np.isnan(X[:, i]), i] = v
        ok = ~np.isnan(X).any(axis=1)
        return np.where(np.isnan(X), 0.0, X), ok

    def distances(self, x: np.ndarray) -> np.ndarray:
        d = np.zeros((len(x), self.H))
        for i in range(self.n_in):  # input by input, as the oracle's per-neuron loop sums them
            d += (x[:, [i]] - self.centers[None, :, i]) ** 2
        return d

    def hidden(self, x: np.ndarray):
        """``(a [rows, H] before the normalisation, c, g, d)``."""
        d = self.distances(x)
        c = self.n_in * np.log(self.altitude)
        g = 1.0 / (2.0 * self.width * self.width)
        return np.exp(c[None] - d / (2.0 * self.width * self.width)[None]), c, g, d

    def tail(self, z: np.ndarray, ok: np.ndarray) -> dict:
        """Output activation, output normalisation and the decode on pre-activations ``z [rows, n_out]``:
        ``out`` (what ``probs`` holds for a classifier, else the activation), ``score``, ``valid``."""
        with np.errstate(all="ignore"):
            f = activate(self.out_act, z, 0.0 if self.out_thr is None else self.out_thr)
            P = normalize_layer(self.final_norm, f)
        if self.classification:
            score = np.argmax(P, axis=1).astype(np.float64)  # a NaN is the maximum, the first of equals wins
            valid = ok.copy()
        else:
            y = P[:, 0]
            valid = ok & np.isfinite(y) & (np.abs(y) <= np.finfo(F32).max)
            score = y
            if self.target is not None:
                score = y * self.target.get("factor", 1.0) + self.target.get("constant", 0.0)
                if self.target.get("cast") == "round":
                    score = np.floor(score + 0.5)
        return dict(z=z, f=f, out=np.where(ok[:, None], P, np.nan), score=np.where(valid, score, np.nan), valid=valid)

    def reference(self, Xi=None) -> dict:
        """The whole network in float64, and the scale ``T [rows, n_out]`` of the bound on ``z``."""
        x, ok = self.inputs(Xi)
        a, c, g, _ = self.hidden(x)
        xc, wc = x - self.mu, self.centers - self.mu  # the expansion runs on the centred values
        D = (xc * xc).sum(1)[:, None] + 2.0 * np.abs(xc) @ np.abs(wc).T + (wc * wc).sum(1)[None]
        aV = np.abs(self.V)
        with np.errstate(all="ignore"):
            if self.hidden_norm in (None, "none"):
                z = a @ self.V.T + self.bias
                T = (a * (1.0 + np.abs(c)[None] + g[None] * D)) @ aV.T + np.abs(z)
            else:
                if self.hidden_norm == "softmax":
                    a_max = float(np.exp(c.max()))
                    e = np.exp(a - a_max)
                    wgt = e * (1.0 + a_max + a * (1.0 + np.abs(c)[None] + g[None] * D))
                else:
                    e, wgt = a, a * (1.0 + np.abs(c)[None] + g[None] * D)
                S = e.sum(axis=1, keepdims=True)
                o = (e @ self.V.T) / S
                z = o + self.bias
                T = (wgt @ aV.T) / S + np.abs(o) * wgt.sum(axis=1, keepdims=True) / S + np.abs(z)
        r = self.tail(z, ok)
        r["T"] = T
        return r


# --------------------------------------------------------------------------- the one-hot probe


def _output_weights(rng, n_out: int, H: int, dups):
    """``V [n_out, H]`` from +-{1, 2, 3}: hidden units 4, 8 or 32 apart never share a weight of any
    output (the rule of ``_exact.int_network``), so swapping two of them shows in every output.
    Biases are integers in -2..2; output ``dst`` of ``dups`` copies ``src`` (equal logits on every row)."""
    V = rng.integers(1, 4, size=(n_out, H)).astype(np.float64) * rng.choice([-1.0, 1.0], size=(n_out, H))
    for u in range(H):
        for o in range(n_out):
            while any(u >= d and V[o, u] == V[o, u - d] for d in (4, 8, 32)):
                V[o, u] = float(rng.integers(1, 4)) * float(rng.choice([-1.0, 1.0]))
    b = rng.integers(-2, 3, size=n_out).astype(np.float64)
    for src, dst in dups:
        V[dst], b[dst] = V[src], b[src]
    return V, b


def duplicates(H: int) -> Dict[int, int]:
    """``{unit: the unit whose centre it repeats}``: every 7th centre is repeated once, 4 further (the
    other lane half of the 32-unit tile) and 32 further (the next tile) in turn. ``grid_centers`` puts
    both copies on one centre; one copy each keeps the simplemax mean over a group a dyadic number."""
    out = {}
    for n, k in enumerate(range(0, H, 7)):
        d = 4 if n % 2 == 0 else 32
        if k + d < H and (k + d) % 7:
            out[k + d] = k
    return out


def onehot_centers(n_in: int, H: int, seed: int, centroid: np.ndarray) -> np.ndarray:
    """Integer centres, distinct but for ``duplicates(H)``, whose column sums are ``H centroid``: their
    mean is the integer vector ``centroid`` exactly. Unit 2 sits on the centroid itself (the one point a
    padded unit, all zeros after centring, would fire on)."""
    rng = np.random.default_rng(seed)
    lo, hi = E.grid_range(H, n_in)
    dup = duplicates(H)
    if H == 1:
        return centroid[None, :].astype(np.float64)
    assert H >= 8, "no unit is free to balance the column sums"
    for _ in range(20):
        seen, rows = {tuple([0] * n_in)}, []
        while len(rows) < H:
            c = tuple(int(v) for v in rng.integers(lo, hi + 1, size=n_in))
            if len(rows) == 2:
                c = tuple([0] * n_in)
            elif c in seen:
                continue
            seen.add(c)
            rows.append(c)
        C = np.array(rows, dtype=np.float64)
        for t, s in dup.items():
            C[t] = C[s]
        free = [j for j in range(H) if j != 2 and j not in dup and j not in dup.values()]
        deficit = -C.sum(axis=0)
        p = 0
        for i in range(n_in):
            for _ in range(int(abs(deficit[i]))):
                C[free[p % len(free)], i] += np.sign(deficit[i])
                p += 1
        heads = [tuple(C[j]) for j in range(H) if j not in dup]
        if len(set(heads)) == len(heads):
            assert not C.sum(axis=0).any()
            return C + centroid[None, :]
    raise AssertionError("no distinct centres found")


def onehot_probe(n_in: int, H: int, n_out: int, seed: int, centroid=None, hidden_norm: Optional[str] = None,
                 classification: bool = False, dups=(), missing: bool = False, **kw) -> Probe:
    """The one-hot probe (module docstring). Rows: every centre; every centre moved one step along one
    input (i cycles; left out where it lands on a centre); the zero row; an all-NaN row; a row of 3e19;
    with ``missing``, ``mapMissingTo`` on the first and the last input, a row with NaN there and its twin
    that holds the replacements (unit 3's centre). The list is repeated to at least 264 rows and rows
    NAN_POSITIONS then become a centre with one NaN. Under ``simplemax`` only rows on a centre, or at least
    6 away from every centre (``g d > 745``: float64 underflows too), are kept: the fp32 underflow between
    is a documented deviation and not this probe's subject.

    ``p.unit [rows]``: the unit whose centre the row is on, -1 where no unit fires."""
    mu = np.zeros(n_in) if centroid is None else np.asarray(centroid, np.float64)
    assert mu.shape == (n_in,) and np.array_equal(mu, np.round(mu))
    C = onehot_centers(n_in, H, seed, mu)
    assert np.array_equal(C.mean(axis=0), mu)
    rng = np.random.default_rng(seed + 4099)
    V, b = _output_weights(rng, n_out, H, dups)
    first = {}
    head = np.array([first.setdefault(tuple(c), j) for j, c in enumerate(C)])  # first unit of every centre
    rows, unit = [c.copy() for c in C], list(head)
    for j in range(H):
        r = C[j].copy()
        r[j % n_in] += 1.0
        if tuple(r) not in first:
            rows.append(r)
            unit.append(-1)
    zero = np.zeros(n_in)
    rows.append(zero)
    unit.append(first.get(tuple(zero), -1))
    rows.append(np.full(n_in, np.nan))
    unit.append(-1)
    rows.append(np.full(n_in, HUGE))
    unit.append(-1)
    map_missing = None
    if missing:
        assert n_in >= 3 and H > 3
        mapped = (0, n_in - 1)
        map_missing = {i: float(C[3, i]) for i in mapped}
        r = C[3].copy()
        r[list(mapped)] = np.nan
        rows += [r, C[3].copy()]
        unit += [int(head[3])] * 2
    X, unit = np.array(rows), np.array(unit)
    if hidden_norm == "simplemax":
        with np.errstate(invalid="ignore"):
            dmin = np.array([np.nan_to_num(((r[None] - C) ** 2).sum(1), nan=np.inf).min() for r in X])
        keep = (unit >= 0) | (dmin >= 6.0)
        X, unit, dmin = X[keep], unit[keep], dmin[keep]
        assert ((unit >= 0) | (128.0 * dmin > 745.0)).all()  # the simplemax condition
    reps = max(2, -(-264 // len(X)))
    X, unit = np.tile(X, (reps, 1)), np.tile(unit, reps)
    free = [i for i in range(n_in) if not (map_missing and i in map_missing)]
    for pos in NAN_POSITIONS:
        X[pos] = C[pos % H]
        X[pos, free[pos % len(free)]] = np.nan
        unit[pos] = -1
    p = Probe(C, np.full(H, 1.0 / 16), np.ones(H), V, b, X.astype(F32), hidden_norm=hidden_norm,
              classification=classification, map_missing=map_missing, **kw)
    p.unit, p.head, p.dup_rows = unit, head, np.isin(unit, [s for s in duplicates(H).values()])
    return p


def onehot_preactivations(p: Probe) -> np.ndarray:
    """``z [rows, n_out]`` of a one-hot probe in closed form: the bias plus the output weights of the
    units on the row's centre, summed (``none``) or averaged (``simplemax``); no unit: the bias alone, or
    0 / 0 under ``simplemax``."""
    z = np.tile(p.bias[None], (len(p.Xi), 1))
    for r, u in enumerate(p.unit):
        if u >= 0:
            group = np.flatnonzero(p.head == u)
            z[r] += p.V[:, group].sum(axis=1) / (len(group) if p.hidden_norm == "simplemax" else 1)
        elif p.hidden_norm == "simplemax":
            z[r] = np.nan
    return z


def onehot_expected(p: Probe) -> dict:
    """``tail`` of the closed-form pre-activations: what a correct kernel returns in every bit."""
    return p.tail(onehot_preactivations(p), p.inputs()[1])


def onehot_guard(p: Probe) -> None:
    """The exactness guard on what the device forms: centred inputs and centres, ``G``, both squared
    norms and ``d`` are integers below 2^24 (the 3e19 row aside, which is infinitely far by design)."""
    x, _ = p.inputs()
    x = x[np.abs(x).max(axis=1) < 1e6]
    xc, wc = x - p.mu, p.centers - p.mu
    G, xx, wn = xc @ wc.T, (xc * xc).sum(1), (wc * wc).sum(1)
    E.assert_exact([xc, wc, G, xx, wn, xx[:, None] - 2.0 * G, xx[:, None] - 2.0 * G + wn[None], p.V, p.bias])


# --------------------------------------------------------------------------- the smooth probe


def smooth_probe(n_in: int, H: int, n_out: int, seed: int, hidden_norm: Optional[str] = None,
                 final_norm: Optional[str] = None, per_unit_altitude: bool = True, rows: int = 257, **kw) -> Probe:
    """Integer centres and inputs in -3..3, widths ``w0 {1/2, 1, 2}`` with ``w0 = 2 sqrt(n_in)`` (the mean
    squared distance is 8 n_in, so ``g d`` is near 4, 1 and 1/4), altitudes 1 or ``1 + k / (32 n_in)``,
    ``k`` in -3..3; output weights as the one-hot probe's. Units 1, 5 and 33 have pairwise different
    widths and altitudes (the c / g / norm swaps of ``panel_mutants`` exchange them). A classifier from
    two outputs on. Row 7 carries a NaN, row 11 is all NaN."""
    rng = np.random.default_rng(seed)
    C = rng.integers(-3, 4, size=(H, n_in)).astype(np.float64)
    w0 = 2.0 * np.sqrt(n_in)
    width = w0 * rng.choice([0.5, 1.0, 2.0], size=H)
    alt = 1.0 + (rng.integers(-3, 4, size=H) / (32.0 * n_in) if per_unit_altitude else np.zeros(H))
    for j, (s, k) in {1: (0.5, 3), 5: (2.0, -3), 33: (1.0, 0)}.items():
        if j < H:
            width[j] = w0 * s
            alt[j] = 1.0 + (k / (32.0 * n_in) if per_unit_altitude else 0.0)
    V, b = _output_weights(rng, n_out, H, ())
    X = rng.integers(-3, 4, size=(rows, n_in)).astype(F32)
    if rows > 11:
        X[7, n_in // 2] = np.nan
        X[11] = np.nan
    return Probe(C, width, alt, V, b, X, hidden_norm=hidden_norm, final_norm=final_norm,
                 classification=n_out > 1, **kw)


BOUND_SHAPES = [(3, 33, 1), (17, 70, 5), (40, 96, 3), (8, 1024, 3), (128, 33, 2)]
BOUND_NORMS = [(None, None), ("simplemax", None), ("softmax", None), (None, "softmax"), ("simplemax", "softmax"),
               ("softmax", "softmax")]


def bound_cases():
    """``(n_in, H, n_out, hidden norm, final norm)``; a final normalisation only on a classifier."""
    return [(n_in, H, n_out, hn, fn) for n_in, H, n_out in BOUND_SHAPES for hn, fn in BOUND_NORMS
            if fn is None or n_out > 1]


def bound_probe(n_in, H, n_out, hn, fn) -> Probe:
    return smooth_probe(n_in, H, n_out, seed=n_in + H, hidden_norm=hn, final_norm=fn)


def check_bound(p: Probe, ref: dict, out: np.ndarray, c: float = None):
    """``(largest ratio, tolerance [rows, n_out])`` of outputs ``out`` against the rule of the smooth probe:
    ``|out - reference| <= C 2^-24 T`` per output and row; after a final softmax a probability is within
    ``2 max_k(C 2^-24 T_k) + SOFTMAX_C 2^-24``. The ratio is the error over the tolerance at C = 1 (for a
    final softmax: what C would have to be)."""
    c = C if c is None else c
    v = ref["valid"]
    err = np.abs(np.asarray(out, np.float64) - ref["out"])[v]
    T = ref["T"][v]
    if p.final_norm == "softmax":
        Tm = T.max(axis=1, keepdims=True)
        tol = 2.0 * c * U * Tm + A.SOFTMAX_C * U + 0.0 * T
        ratio = np.maximum(err - A.SOFTMAX_C * U, 0.0) / (2.0 * U * Tm)
    else:
        tol = c * U * T
        ratio = err / (U * T)
    full = np.full(ref["T"].shape, np.inf)
    full[v] = tol
    return float(ratio.max(initial=0.0)), full


def clear_rows(p: Probe, ref: dict, tol: np.ndarray) -> np.ndarray:
    """Valid rows whose two largest reference outputs are more than twice the tolerance apart."""
    top = np.sort(np.where(np.isnan(ref["out"]), -np.inf, ref["out"]), axis=1)
    return ref["valid"] & (top[:, -1] - top[:, -2] > 2.0 * tol.max(axis=1))


# --------------------------------------------------------------------------- packed panels: un-packer, twin, mutants


def acc_unit(r, h):
    """rbf.hip ``acc_row``: the unit of a 32 x 32 accumulator tile that register r of lane half h holds."""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def unpack_panels(pan: np.ndarray, kp: int):
    """``(W [tiles 32, kp], V [32, tiles 32], c, g, wn)`` of the panels as rbf.hip reads them: float4
    ``q 64 + lane`` of the centre fragments is unit ``lane & 31``, inputs ``8 q + 4 (lane >> 5) + e``; float4
    ``r4 64 + lane`` of the V slice is output ``lane & 31``, units ``acc_row(4 r4 + e, lane >> 5)``; then
    ``c | g | wn``, each as ``[h][r]`` in ``acc_row`` order."""
    pan = np.asarray(pan, F32).reshape(-1, kp * 32 + TAIL)
    tiles = len(pan)
    W, V = np.zeros((tiles * 32, kp), F32), np.zeros((32, tiles * 32), F32)
    consts = np.zeros((3, tiles * 32), F32)
    for t in range(tiles):
        for lane in range(64):
            m, h = lane & 31, lane >> 5
            for q in range(kp // 8):
                W[32 * t + m, 8 * q + 4 * h: 8 * q + 4 * h + 4] = pan[t, 4 * (q * 64 + lane): 4 * (q * 64 + lane) + 4]
            for r4 in range(4):
                for e in range(4):
                    V[m, 32 * t + acc_unit(4 * r4 + e, h)] = pan[t, kp * 32 + 4 * (r4 * 64 + lane) + e]
        for i in range(3):
            for h in range(2):
                for r in range(16):
                    consts[i, 32 * t + acc_unit(r, h)] = pan[t, kp * 32 + 1024 + 32 * i + 16 * h + r]
    return W, V, consts[0], consts[1], consts[2]


def twin(plan, X: np.ndarray, pan: Optional[np.ndarray] = None) -> dict:
    """The device's formula in fp32 numpy over an ``RbfPlan``'s tensors (``pan``: its panels, mutated):
    the input stage, distances by expansion with the clamp, fp32 ``exp``, plain in-order fp32 sums, the
    division by the hidden sum after the output product. Returns ``z`` (the pre-activations with the bias)
    and ``bad`` (rows with a missing input); :func:`twin_outputs` finishes them."""
    t = lambda a: np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    pan = t(plan.panels) if pan is None else pan
    W, V, c, g, wn = unpack_panels(pan, plan.kp)
    sc, sh, ms, ix = t(plan.in_scale), t(plan.in_shift), t(plan.in_missing), t(plan.in_index)
    x = np.asarray(X, F32)[:, ix]
    with np.errstate(all="ignore"):
        y = np.where(np.isnan(x), ms[None], (x.astype(np.float64) * sc + sh).astype(F32))  # one fma
        bad = np.isnan(y).any(axis=1)
        y = np.where(np.isnan(y), F32(0), y).astype(F32)
        xx = np.zeros(len(y), F32)
        G = np.zeros((len(y), len(W)), F32)
        for k in range(plan.n_in):
            xx = xx + y[:, k] * y[:, k]
            G = G + y[:, [k]] * W[None, :, k]
        d = (xx[:, None] - F32(2) * G) + wn[None]
        d = np.where(d < 0, F32(0), d)
        d = np.where(np.isnan(d), F32(np.inf), d).astype(F32)
        a = np.exp((c[None] - g[None] * d).astype(F32)).astype(F32)
        if plan.hidden_norm == 1:
            a = np.where(np.isinf(wn)[None], F32(0), np.exp(a - F32(plan.a_max))).astype(F32)
        s = np.zeros(len(y), F32)
        out = np.zeros((len(y), 32), F32)
        for j in range(len(W)):
            s = s + a[:, j]
            out = out + a[:, [j]] * V[None, :, j]
        if plan.hidden_norm != 0:
            out = out / s[:, None]
        z = out + t(plan.out_bias)[None]
    return dict(z=z[:, :plan.n_out].astype(F32), bad=bad)


def twin_outputs(p: Probe, tw: dict) -> dict:
    """The output activation, normalisation and decode of the twin's ``z``, in fp32: ``out``, ``score``, ``valid``."""
    z = tw["z"]
    with np.errstate(all="ignore"):
        f = A.twin_activate(p.out_act, z, 0.0 if p.out_thr is None else p.out_thr).astype(F32)
        if p.final_norm == "softmax":
            e = np.exp(f - f.max(axis=1, keepdims=True)).astype(F32)
            s = np.zeros(len(e), F32)
            for k in range(e.shape[1]):
                s = s + e[:, k]
            f = e / s[:, None]
    ok = ~tw["bad"]
    if p.classification:
        score, valid = np.argmax(f, axis=1).astype(np.float64), ok
    else:
        valid = ok & np.isfinite(f[:, 0])
        score = f[:, 0].astype(np.float64)
        if p.target is not None:
            score = score * p.target.get("factor", 1.0) + p.target.get("constant", 0.0)
            score = np.floor(score + 0.5) if p.target.get("cast") == "round" else score
    return dict(out=np.where(ok[:, None], f, np.nan), score=np.where(valid, score, np.nan), valid=valid)


# names of the mutants only a smooth probe can show: every one-hot unit has c = 0 and g = 128
SMOOTH_ONLY = ("swap-c-", "swap-g-")


def panel_mutants(kp: int, H: int, n_out: int) -> Dict[str, callable]:
    """Named mutants of an ``RbfPlan``'s ``panels`` as ``[tiles, kp 32 + TAIL]`` float32 (modified in
    place; positions from rbf.hip's index maps). Units 1 and 5 (the two lane halves) and 1 and 33 (two
    tiles) are exchanged in the centre fragments, in the V slice and in each of c, g and the squared norm;
    input columns 0 and 4 (lane halves) and 0 and 8 (k-step groups) in the centre fragments; the last real
    unit loses its output weights; the first padded unit gets the squared norm 0. A mutant the shape
    cannot hold is left out."""
    def frag(u, k):  # float position of centre entry (unit u, input k)
        q, h, e = k // 8, (k % 8) // 4, k % 4
        return u // 32, 4 * (q * 64 + 32 * h + u % 32) + e

    def vpos(o, u):  # float position of output weight (output o, unit u)
        m = u % 32
        h = (m >> 2) & 1
        r = (m & 3) + 4 * (m >> 3)
        return u // 32, kp * 32 + 4 * ((r >> 2) * 64 + 32 * h + o) + (r & 3)

    def cpos(i, u):  # float position of constant i (0 c, 1 g, 2 squared norm) of unit u
        m = u % 32
        h = (m >> 2) & 1
        return u // 32, kp * 32 + 1024 + 32 * i + 16 * h + (m & 3) + 4 * (m >> 3)

    def swap(pan, a, b):
        pan[a], pan[b] = pan[b], pan[a]

    def swap_centres(u, v):
        def f(pan):
            for k in range(kp):
                swap(pan, frag(u, k), frag(v, k))
        return f

    def swap_v(u, v):
        def f(pan):
            for o in range(32):
                swap(pan, vpos(o, u), vpos(o, v))
        return f

    def swap_const(i, u, v):
        return lambda pan: swap(pan, cpos(i, u), cpos(i, v))

    def swap_cols(k0, k1):
        def f(pan):
            for u in range(H):
                swap(pan, frag(u, k0), frag(u, k1))
        return f

    def zero_v(pan):
        for o in range(32):
            pan[vpos(o, H - 1)] = 0.0

    def padded_norm(pan):
        pan[cpos(2, H)] = 0.0

    out = {}
    for u, v, name in ((1, 5, "4-apart"), (1, 33, "32-apart")):
        if v < H:
            out[f"swap-centres-{name}"] = swap_centres(u, v)
            out[f"swap-V-{name}"] = swap_v(u, v)
            for i, what in enumerate(("c", "g", "norm")):
                out[f"swap-{what}-{name}"] = swap_const(i, u, v)
    if H > 1:  # one unit at centre 0: an exchange of its columns is no change
        if kp > 4:
            out["swap-input-columns-4-apart"] = swap_cols(0, 4)
        if kp > 8:
            out["swap-input-columns-8-apart"] = swap_cols(0, 8)
    out["zero-last-unit-V"] = zero_v
    if H % 32:
        out["padded-unit-finite-norm"] = padded_norm
    return out


def mutate(plan, f) -> np.ndarray:
    """Apply mutant ``f`` to the plan's panels in place of the tensor; returns the original to put back."""
    orig = plan.panels.cpu().numpy().copy()
    pan = orig.reshape(plan.n_tiles, -1).copy()
    f(pan)
    plan.panels = plan._t(pan.reshape(-1))
    return orig


def restore(plan, orig: np.ndarray) -> None:
    plan.panels = plan._t(orig)


# --------------------------------------------------------------------------- the exact cases (CPU and GPU files)

# (n_in, H, n_out): the input buckets 16|17, 32|33, 64|65 and 128, hidden tiles 31 / 32 / 33, 64 / 65,
# one and 32 outputs, 32 tiles over a short panel
EXACT_SHAPES = [(1, 1, 1), (16, 31, 1), (17, 32, 2), (32, 33, 31), (33, 64, 32), (64, 65, 3), (65, 96, 1),
                (128, 33, 2), (8, 1024, 3)]
HIDDEN_NORMS = (None, "simplemax")
ROUTE_SHAPES = [(16, 31, 1), (17, 32, 2)]  # n_in % 4 == 0, and not
MUTANT_SHAPES = [(17, 70, 3), (33, 64, 32)]
ACT_SHAPE = (17, 32, 2)


def output_dups(n_out: int):
    """Output neurons that copy another one: 4 apart (the two lane halves of the decode) and neighbours."""
    return tuple(d for d in ((1, 5), (8, 9)) if d[1] < n_out)


def exact_probe(n_in, H, n_out, hidden_norm, **kw) -> Probe:
    """The one-hot probe of an EXACT_SHAPES entry: a classifier without an output normalisation from
    two outputs on (``probs`` are the integer logits), else a regression."""
    return onehot_probe(n_in, H, n_out, seed=n_in + H, hidden_norm=hidden_norm, classification=n_out > 1,
                        dups=output_dups(n_out), **kw)


def activation_probe(act: str) -> Probe:
    """ACT_SHAPE as a two-output classifier without normalisation: ``probs`` are ``f(z)`` of both outputs."""
    n_in, H, n_out = ACT_SHAPE
    p = onehot_probe(n_in, H, n_out, seed=n_in + H, classification=True, out_act=act)
    if act == "reciprocal":
        p.bias = p.bias + A.POLE_SHIFT
    if act == "threshold":
        p.out_thr = float(p.bias[0])  # a row no unit fires on sits exactly on it
    return p


# (n_in, H, n_out, hidden norm, True): a non-zero centroid with ``mapMissingTo`` on two inputs
CENTROID_CASES = [(17, 32, 2, None, True), (32, 33, 31, "simplemax", True)]


def target_probe() -> Probe:
    n_in, H, n_out = ROUTE_SHAPES[0]
    return exact_probe(n_in, H, n_out, None, target=dict(factor=2.0, constant=-1.0, cast="round"))


def nonzero_centroid(n_in: int) -> np.ndarray:
    return np.array([(3, -2, 1)[i % 3] for i in range(n_in)], np.float64)


def permutation(n: int, seed: int = 1) -> list:
    """A permutation of the fields without a fixed point (from two fields on): one random cycle."""
    cycle = np.random.default_rng(seed).permutation(n)
    out = np.empty(n, int)
    out[cycle] = np.roll(cycle, 1)
    return out.tolist()
