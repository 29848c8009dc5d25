"""Exact-eta probes for the score epilogue (csrc/epilogue.h, common.h::apply_link) and linear.hip.

Coefficients come from {+-0.5, +-1, +-2}, intercepts are small integers and inputs lie on the grid
of multiples of 1/8, so every linear predictor eta_k is an exact fp32 number in any summation order,
fused or not. The float64 oracle, the float64 reference below (written without reading
models/regression.py: cancellation-free link forms), the fp32 twin of the epilogue and the kernel
then start from the same bits, and labels, validity and cast Target values compare for equality on
every row.

Layout of a steerable document (``F >= 2 K``, or one table): field k is the carrier of table k and
field K + k its anti-carrier. Both hold the same value v_k; in table k both have the coefficient
s_k / 2 (s_k = +-1), in every other table j the two coefficients are w and -w, so v_k reaches no
eta but its own. The other fields are fillers (multiples of 1/4, any coefficient of the set); the
carrier absorbs their contribution, which puts eta_k on a chosen target. A sparse document
(``sparse=True``) has table k list only the fields f = k (mod K); field k is its carrier."""

import io
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
from scipy import special

from flink_jpmml_amd.bench.synth import _data_dictionary, _header, _mining_schema

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = float(np.finfo(F32).tiny)
INF = float("inf")
COEFS = (0.5, -1.0, 2.0, -0.5, 1.0, -2.0)
LINKS = ("none", "logit", "exp", "probit", "cloglog", "loglog", "cauchit")
LINK_ID = {"none": 0, "logit": 1, "exp": 2, "probit": 3, "cloglog": 4, "loglog": 5, "cauchit": 6}
BOUNDED = ("logit", "probit", "cloglog", "loglog", "cauchit")
MODE_AFFINE, MODE_LOGISTIC2, MODE_ARGMAX, MODE_SOFTMAX, MODE_CUMULATIVE, MODE_LINKMAX = range(6)

# every multiple of 1/8 in [-12, 12], then the saturation points of the links in fp32 and float64
SWEEP = np.concatenate([np.arange(-96, 97) / 8.0,
                        [s * t for t in (17, 20, 30, 37, 40, 50, 88, 89, 100, 104, 120) for s in (1, -1)]])
# (eta_a, eta_b) of two classes: fp32 saturates both, float64 still orders the first three
PAIRS = ((20.0, 30.0), (30.0, 20.0), (40.0, 50.0), (-120.0, -100.0), (-100.0, -120.0))


def _num(v) -> str:
    v = float(v)
    return str(int(v)) if v == int(v) else repr(v)


def class_labels(K: int) -> list:
    """Numeric labels that are not the class index: a score names the label-table entry."""
    return [str(10 * (k + 1)) for k in range(K)]


# --------------------------------------------------------------------------- documents


class Probe:
    """A ``RegressionModel`` with ``F`` fields and ``K`` tables (0: one regression table)."""

    def __init__(self, F: int, K: int = 0, norm: str = "none", sparse: bool = False,
                 zero_coef: Optional[Tuple[int, int]] = None, target: Optional[dict] = None):
        self.F, self.K, self.norm, self.sparse, self.target = F, K, norm, sparse, target
        T = self.T = max(K, 1)
        self.W = np.zeros((F, T))
        self.listed = np.zeros((F, T), dtype=bool)
        self.b = np.array([float(k % 5 - 2) for k in range(T)])
        self.sign = np.array([1.0 if k % 2 == 0 else -1.0 for k in range(T)])
        self.steerable = sparse or T == 1 or F >= 2 * T
        if sparse:
            assert F >= T
            for f in range(F):
                self.W[f, f % T] = COEFS[f % 6]
                self.listed[f, f % T] = True
            self.carrier = np.array([COEFS[k % 6] for k in range(T)])
            self.fillers = list(range(T, F))
        elif T == 1:
            self.listed[:] = True
            self.W[0, 0] = -1.0
            self.W[1:, 0] = [COEFS[f % 6] for f in range(1, F)]
            self.carrier = np.array([-1.0])
            self.fillers = list(range(1, F))
        else:
            self.listed[:] = True
            for f in range(F):
                self.W[f] = [COEFS[(f + 2 * k) % 6] for k in range(T)]
            if self.steerable:
                for k in range(T):
                    self.W[T + k] = -self.W[k]
                    self.W[k, k] = self.W[T + k, k] = self.sign[k] / 2
            self.carrier = self.sign.copy()
            self.fillers = list(range(2 * T, F)) if self.steerable else []
        if zero_coef is not None:  # an explicit coefficient="0": listed, so 0 * inf = NaN as in the oracle
            f, k = zero_coef
            assert not self.listed[f, k]
            self.listed[f, k] = True

    # -- document
    def pmml(self) -> str:
        out = io.StringIO()
        _header(out, f"exact-eta regression {self.F} x {self.K} {self.norm}")
        cats = class_labels(self.K) if self.K else None
        _data_dictionary(out, self.F, "y", "integer" if self.K else "double", cats)
        fn = "classification" if self.K else "regression"
        out.write(f' <RegressionModel functionName="{fn}" normalizationMethod="{self.norm}">\n')
        _mining_schema(out, self.F, "y", "  ")
        if self.target:
            out.write("  " + target_xml(**self.target) + "\n")
        for k in range(self.T):
            tc = f' targetCategory="{cats[k]}"' if cats else ""
            out.write(f'  <RegressionTable intercept="{_num(self.b[k])}"{tc}>')
            out.write("".join(f'<NumericPredictor name="f{f}" coefficient="{_num(self.W[f, k])}"/>'
                              for f in range(self.F) if self.listed[f, k]))
            out.write('</RegressionTable>\n')
        out.write(' </RegressionModel>\n</PMML>\n')
        return out.getvalue()

    # -- inputs
    def steer(self, targets: np.ndarray, seed: int = 0, nan_every: int = 41) -> np.ndarray:
        """fp32 inputs that put eta_k of row r on ``targets[r, k]`` (+-inf allowed where the carrier
        reaches one table only), followed by a copy of every ``nan_every``-th row from row 7 with
        one cell missing (appended, so that no constructed row is lost)."""
        assert self.steerable
        targets = np.asarray(targets, np.float64).reshape(len(targets), self.T)
        rng = np.random.default_rng(seed)
        X = np.zeros((len(targets), self.F))
        if self.fillers:
            X[:, self.fillers] = rng.integers(-8, 9, size=(len(targets), len(self.fillers))) / 4.0
        r = np.where(self.listed, self.W, 0.0)[self.fillers].T @ X[:, self.fillers].T  # [T, n]
        v = (targets - self.b[None, :] - r.T) / self.carrier[None, :]
        if not self.sparse and self.T > 1:
            assert np.isfinite(v).all(), "an infinite carrier would meet its anti-carrier: inf - inf"
            X[:, self.T:2 * self.T] = v
        X[:, :self.T] = v
        assert np.array_equal(X.astype(F32).astype(np.float64), X, equal_nan=True)
        return with_missing_rows(X.astype(F32), nan_every)

    # -- float64 linear predictors from the builder's own arrays, with the exactness guard
    def eta(self, X: np.ndarray, guard: bool = True, unguarded: Optional[np.ndarray] = None):
        """``(eta [rows, T] float64, missing [rows])``. Asserts ``float32(eta) == eta`` and the same
        for every partial sum in field order and in reverse (``unguarded``: rows that hold FLT_MAX
        or infinite cells on purpose)."""
        X = np.asarray(X, np.float64)
        miss = np.isnan(X).any(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            terms = np.where(self.listed[None], X[:, :, None] * self.W[None], 0.0)  # [rows, F, T]
            eta = self.b[None, :] + terms.sum(axis=1)
            if guard:
                rows = ~miss & np.isfinite(X).all(axis=1)
                if unguarded is not None:
                    rows &= ~unguarded
                for order in (terms[rows], terms[rows][:, ::-1]):
                    part = self.b[None, None, :] + np.cumsum(order, axis=1)
                    assert np.array_equal(part.astype(F32).astype(np.float64), part), "partial sum is not exact in fp32"
                    assert np.array_equal(order.astype(F32).astype(np.float64), order)
                assert np.array_equal(np.round(eta[rows] * 16) / 16, eta[rows])
        return eta, miss


def with_missing_rows(X: np.ndarray, nan_every: int = 41) -> np.ndarray:
    if not nan_every or len(X) <= 7:
        return X
    M = X[7::nan_every].copy()
    for j, i in enumerate(range(7, len(X), nan_every)):
        M[j, (3 * i) % X.shape[1]] = np.nan
    return np.concatenate([X, M])


def target_xml(min=None, max=None, factor=1.0, constant=0.0, cast=None, default=None) -> str:
    attrs = f'field="y" rescaleFactor="{_num(factor)}" rescaleConstant="{_num(constant)}"'
    if min is not None:
        attrs += f' min="{_num(min)}"'
    if max is not None:
        attrs += f' max="{_num(max)}"'
    if cast is not None:
        attrs += f' castInteger="{cast}"'
    body = f'<TargetValue defaultValue="{_num(default)}"/>' if default is not None else ""
    return f'<Targets><Target {attrs}>{body}</Target></Targets>'


def glm_doc(kind: str, link: str, F: int, cuts: Sequence[float] = (), reference_first: bool = False) -> str:
    """``GeneralRegressionModel`` over numeric covariates only (parameter p<j> is field f<j>, slopes
    cycle through the coefficient set; field 0 has slope 1). ``ordinal``: ``len(cuts) + 1`` ordered
    categories, ``link`` the cumulativeLink; ``binomial``: categories 10 / 20, event 20."""
    out = io.StringIO()
    _header(out, f"exact-eta GLM {kind} {link}")
    J = len(cuts) + 1 if kind == "ordinal" else 2
    cats = class_labels(J)
    if kind == "binomial" and reference_first is False:
        cats = cats[::-1]  # event first
    _data_dictionary(out, F, "y", "integer", cats)
    if kind == "ordinal":
        attrs = f'modelType="ordinalMultinomial" cumulativeLink="{link}"'
    else:
        attrs = f'modelType="generalizedLinear" linkFunction="{link}" targetReferenceCategory="10"'
    out.write(f' <GeneralRegressionModel functionName="classification" {attrs}>\n')
    _mining_schema(out, F, "y", "  ")
    params = ["p0"] + [f"p{j + 1}" for j in range(F)]
    out.write('  <ParameterList>' + "".join(f'<Parameter name="{p}"/>' for p in params) + '</ParameterList>\n')
    out.write('  <CovariateList>' + "".join(f'<Predictor name="f{j}"/>' for j in range(F)) + '</CovariateList>\n')
    out.write('  <PPMatrix>' + "".join(f'<PPCell value="1" predictorName="f{j}" parameterName="p{j + 1}"/>'
                                       for j in range(F)) + '</PPMatrix>\n  <ParamMatrix>\n')
    if kind == "ordinal":
        for c, cut in zip(cats[:-1], cuts):
            out.write(f'   <PCell parameterName="p0" targetCategory="{c}" beta="{_num(cut)}"/>\n')
        tc = ""
    else:
        out.write('   <PCell parameterName="p0" targetCategory="20" beta="0"/>\n')
        tc = ' targetCategory="20"'
    for j in range(F):
        out.write(f'   <PCell parameterName="p{j + 1}"{tc} beta="{_num(glm_slope(j))}"/>\n')
    out.write('  </ParamMatrix>\n </GeneralRegressionModel>\n</PMML>\n')
    return out.getvalue()


def glm_slope(j: int) -> float:
    return 1.0 if j == 0 else COEFS[j % 6]


def glm_inputs(targets: np.ndarray, F: int, seed: int = 0, nan_every: int = 41) -> Tuple[np.ndarray, np.ndarray]:
    """``(X fp32, shared float64)``: the shared linear predictor sum_j slope_j x_j lands on ``targets``."""
    rng = np.random.default_rng(seed)
    X = np.zeros((len(targets), F))
    X[:, 1:] = rng.integers(-8, 9, size=(len(targets), F - 1)) / 4.0
    slopes = np.array([glm_slope(j) for j in range(F)])
    X[:, 0] = targets - X[:, 1:] @ slopes[1:]
    part = np.cumsum(X * slopes[None], axis=1)
    assert np.array_equal(part.astype(F32).astype(np.float64), part)
    assert np.array_equal(X.astype(F32).astype(np.float64), X, equal_nan=True)
    X = with_missing_rows(X.astype(F32), nan_every)
    return X, (X.astype(np.float64) @ slopes)  # NaN where a cell is missing


# --------------------------------------------------------------------------- float64 reference


def ref_link(name: str, eta: np.ndarray) -> np.ndarray:
    """Cancellation-free float64 forms."""
    eta = np.asarray(eta, np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if name == "none":
            return eta.copy()
        if name == "logit":
            return 1.0 / (1.0 + np.exp(-eta))
        if name == "exp":
            return np.exp(eta)
        if name == "probit":
            return 0.5 * special.erfc(-eta / math.sqrt(2.0))
        if name == "cloglog":
            return -np.expm1(-np.exp(eta))
        if name == "loglog":
            return np.exp(-np.exp(-eta))
        if name == "cauchit":
            return 0.5 + np.arctan(eta) / math.pi
    raise ValueError(name)


def first_max(P: np.ndarray) -> np.ndarray:
    """The oracle's tie rule: NaN counts as -inf, the first maximum wins."""
    return np.argmax(np.where(np.isnan(P), -INF, P), axis=1)


def beyond_fp32(v: np.ndarray) -> np.ndarray:
    """Finite in float64, beyond +-FLT_MAX: fp32 holds an infinity there."""
    v = np.asarray(v, np.float64)
    return np.isfinite(v) & (np.abs(v) > FLT_MAX)


def ref_target(v: np.ndarray, ok: np.ndarray, t: Optional[dict]):
    """clip -> rescale -> floor(v + 0.5) / ceil / floor -> default, in float64."""
    if not t:
        return v, ok
    v = np.asarray(v, np.float64).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if t.get("min") is not None:
            v = np.where(v < t["min"], t["min"], v)
        if t.get("max") is not None:
            v = np.where(v > t["max"], t["max"], v)
        v = v * t.get("factor", 1.0) + t.get("constant", 0.0)
        cast = t.get("cast")
        v = {"round": lambda z: np.floor(z + 0.5), "ceiling": np.ceil, "floor": np.floor, None: lambda z: z}[cast](v)
    if t.get("default") is not None:
        return np.where(ok, v, t["default"]), np.ones_like(ok)
    return v, ok


def reference(eta: np.ndarray, miss: np.ndarray, K: int, norm: str, target: Optional[dict] = None,
              fp32_rule: bool = False, labels: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """Float64 epilogue of ``eta [rows, max(K, 1)]``: ``score`` (regression value / numeric class
    label, NaN where invalid), ``valid``, ``label``, ``probs`` (regression: the link value before the
    Target stage) and ``flagged`` — the rows of the fp32 model-value rule: a float64 model value
    (eta, a link value) beyond +-FLT_MAX, which is an infinity on the device, hence no prediction.
    With ``fp32_rule`` those rows are invalid here too (a regression Target default then applies)."""
    eta = np.asarray(eta, np.float64)
    n = len(eta)
    ok = ~np.asarray(miss, bool)

    def probabilities(eta):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if K == 0:
                return ref_link(norm, eta[:, :1])
            if norm == "softmax":
                E = np.exp(eta - eta.max(axis=1, keepdims=True))
                return E / E.sum(axis=1, keepdims=True)
            if norm == "simplemax":
                return eta / eta.sum(axis=1, keepdims=True)
            if norm.startswith("cumulative:"):
                cum = ref_link(norm.split(":", 1)[1], eta)
                cum[:, -1] = 1.0
                return np.diff(cum, axis=1, prepend=0.0)
            if K == 2:
                p0 = ref_link(norm, eta[:, 0])
                return np.stack([p0, 1.0 - p0], axis=1)
            return ref_link(norm, eta)

    def as_fp32_holds(v):
        return np.where(beyond_fp32(v), np.sign(v) * INF, v)

    P = probabilities(eta)
    finite = np.isfinite(P).all(axis=1)
    # what the device can know: eta as fp32 holds it (an infinity beyond FLT_MAX), then its value likewise
    on_device = np.isfinite(as_fp32_holds(probabilities(as_fp32_holds(eta)))).all(axis=1)
    flagged = ok & finite & ~on_device
    valid = ok & finite
    if fp32_rule:
        valid &= ~flagged
    if K == 0:
        value, valid = ref_target(P[:, 0], valid, target)
        return dict(score=np.where(valid, value, np.nan), valid=valid, label=np.zeros(n, np.int64), probs=P,
                    flagged=flagged)
    label = first_max(P)
    table = np.array([float(s) for s in (labels or class_labels(K))])
    return dict(score=np.where(valid, table[label], np.nan), valid=valid, label=label, probs=P, flagged=flagged)


def epilogue_mode(K: int, norm: str) -> int:
    if K == 0:
        return MODE_AFFINE
    if norm == "softmax":
        return MODE_SOFTMAX
    if norm == "simplemax":
        return MODE_ARGMAX
    if norm.startswith("cumulative:"):
        return MODE_CUMULATIVE
    return MODE_LOGISTIC2 if K == 2 else MODE_LINKMAX


# --------------------------------------------------------------------------- fp32 twin of epilogue.h


def twin_link(link: str, y: np.ndarray, mutant: str = "") -> np.ndarray:
    """``common.h::apply_link`` in numpy fp32 (the library functions differ from the device's in the
    last bits; labels, validity and cast values do not depend on those)."""
    y = np.asarray(y, F32)
    if mutant == "cloglog-loglog-swapped":
        link = {"cloglog": "loglog", "loglog": "cloglog"}.get(link, link)
    one, half = F32(1), F32(0.5)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if link == "logit":
            return (one / (one + np.exp(-y))).astype(F32)
        if link == "exp":
            return np.exp(y).astype(F32)
        if link == "probit":
            s = y if mutant == "probit-sign-dropped" else -y
            return (half * special.erfc(s * F32(0.70710678118654752))).astype(F32)
        if link == "cloglog":
            return (one - np.exp(-np.exp(y))).astype(F32)
        if link == "loglog":
            return np.exp(-np.exp(-y)).astype(F32)
        if link == "cauchit":
            return (half + np.arctan(y) * F32(0.31830988618379067)).astype(F32)
    return y


def oracle_form_link(link: str, y: np.ndarray) -> np.ndarray:
    """``epilogue.h::apply_link_f64``: the float64 forms the oracle itself uses (they saturate where
    it does), for the tie-break of classes that share one fp32 value."""
    y = np.asarray(y, np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if link == "logit":
            return 1.0 / (1.0 + np.exp(-y))
        if link == "exp":
            return np.exp(y)
        if link == "probit":
            return 0.5 * (1.0 + special.erf(y / math.sqrt(2.0)))
        if link == "cloglog":
            return 1.0 - np.exp(-np.exp(y))
        if link == "loglog":
            return np.exp(-np.exp(-y))
        if link == "cauchit":
            return 0.5 + np.arctan(y) / math.pi
    return y


def twin_target(s: np.ndarray, t: Optional[dict], mutant: str = "") -> np.ndarray:
    """``apply_target``: float64 arithmetic on the fp32 model value, result rounded to fp32."""
    v = np.asarray(s, F32).astype(np.float64)
    if not t:
        return v.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        def clip(z):
            if t.get("min") is not None:
                z = np.where(z < t["min"], t["min"], z)
            if t.get("max") is not None:
                z = np.where(z > t["max"], t["max"], z)
            return z

        def rescale(z):
            return z * t.get("factor", 1.0) + t.get("constant", 0.0)

        v = clip(rescale(v)) if mutant == "rescale-before-clip" else rescale(clip(v))
        cast = t.get("cast")
        if cast == "round":
            v = np.rint(v) if mutant == "round-half-even" else np.floor(v + 0.5)
        elif cast == "ceiling":
            v = np.ceil(v)
        elif cast == "floor":
            v = np.floor(v)
        return v.astype(F32)


def _first_max32(P: np.ndarray, last: bool = False) -> np.ndarray:
    Q = np.where(np.isnan(P), -INF, P)
    if last:
        return P.shape[1] - 1 - np.argmax(Q[:, ::-1], axis=1)
    return np.argmax(Q, axis=1)


def twin_epilogue(eta: np.ndarray, row_ok: np.ndarray, K: int, norm: str, target: Optional[dict] = None,
                  a: float = 1.0, b: float = 0.0, thr: float = 0.5, labels: Optional[Sequence[str]] = None,
                  mutant: str = "") -> Dict[str, np.ndarray]:
    """``apply_epilogue`` (and linear.hip's simplemax division) on fp32 accumulators ``eta``."""
    with np.errstate(over="ignore"):
        acc = np.asarray(eta, np.float64).astype(F32)
    n = len(acc)
    ok = np.asarray(row_ok, bool).copy()
    mode = epilogue_mode(K, norm)
    link = norm.split(":", 1)[1] if norm.startswith("cumulative:") else norm
    last = mutant == "argmax-last-maximum"
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if mode == MODE_AFFINE:
            z = (F32(a) * acc[:, 0] + F32(b)).astype(F32)  # exact probes: fused or not is the same number
            s = twin_link(link, z, mutant)
            ok &= np.isfinite(s)
            P = s[:, None].copy()
            v = twin_target(s, target, mutant)
            if target and target.get("default") is not None:
                d = F32(target["default"])
                if mutant == "default-value-cast":
                    d = twin_target(np.array([d]), dict(cast=target.get("cast")))[0]
                v = np.where(ok, v, d)
                ok = np.ones(n, bool)
            return dict(score=np.where(ok, v, F32(np.nan)).astype(F32), valid=ok, label=np.zeros(n, np.int64),
                        probs=P)
        if mode == MODE_LOGISTIC2:
            p0 = twin_link(link, acc[:, 0], mutant)
            if mutant == "one-minus-p0-swapped":
                p0 = (F32(1) - p0).astype(F32)
            label = np.where(p0 > F32(thr) if mutant == "threshold-greater-than" else p0 >= F32(thr), 0, 1)
            P = np.stack([p0, (F32(1) - p0).astype(F32)], axis=1)
            ok &= np.isfinite(p0)
        elif mode == MODE_LINKMAX:
            P = twin_link(link, acc, mutant)
            label = _first_max32(P, last)
            ok &= np.isfinite(P[np.arange(n), label]) if mutant == "validity-from-best-class" \
                else np.isfinite(P).all(axis=1)
            Pd = oracle_form_link(link, acc.astype(np.float64))
        elif mode == MODE_CUMULATIVE:
            cum = twin_link(link, acc, mutant)
            cumd = oracle_form_link(link, acc.astype(np.float64))
            if mutant != "last-cumulative-not-one":
                cum[:, -1] = 1.0
                cumd[:, -1] = 1.0
            P = np.diff(cum, axis=1, prepend=F32(0)).astype(F32)
            Pd = np.diff(cumd, axis=1, prepend=0.0)
            label = _first_max32(P, last)
            ok &= ~np.isnan(P).any(axis=1)
        else:
            if mode == MODE_ARGMAX:  # linear.hip: acc /= sum before the epilogue
                s = np.zeros(n, F32)
                for k in range(acc.shape[1]):
                    s = (s + acc[:, k]).astype(F32)
                acc = (acc / s[:, None]).astype(F32)
                P = acc
                fin = np.isfinite(acc).all(axis=1)
            else:
                mx = np.fmax.reduce(acc, axis=1)
                E = np.exp((acc - mx[:, None]).astype(F32)).astype(F32)
                P = (E / E.sum(axis=1, dtype=np.float64).astype(F32)[:, None]).astype(F32)  # float64 sum, rounded once
                fin = (acc < INF).all(axis=1)
            label = _first_max32(acc, last)
            best = acc[np.arange(n), label]
            if mutant == "validity-from-best-class":
                ok &= ~np.isnan(best) & (best > -INF)
            else:
                ok &= fin & (best > -INF)
        if mode in (MODE_LINKMAX, MODE_CUMULATIVE) and not last:
            # classes that share the largest fp32 value are compared in float64
            best = P[np.arange(n), label]
            tied = (P == best[:, None])
            rows = tied.sum(axis=1) > 1
            label = np.where(rows, first_max(np.where(tied, Pd, -INF)), label)
    table = np.array([float(s) for s in (labels or class_labels(K))], F32)
    s = table[label]
    ok &= ~np.isnan(s)
    return dict(score=np.where(ok, s, F32(np.nan)).astype(F32), valid=ok, label=label, probs=P)


MUTANTS = ("argmax-last-maximum", "threshold-greater-than", "one-minus-p0-swapped", "last-cumulative-not-one",
           "cloglog-loglog-swapped", "probit-sign-dropped", "round-half-even", "rescale-before-clip",
           "default-value-cast", "validity-from-best-class")


# --------------------------------------------------------------------------- grids


def sweep_targets(T: int, base: Sequence[float] = (0.0, -1.0)) -> np.ndarray:
    """Every class in turn runs through ``SWEEP`` while the others rest on ``base`` (cycled)."""
    rows = []
    for k in range(T):
        t = np.array([base[(j + (j > k)) % len(base)] if j != k else 0.0 for j in range(T)])
        block = np.tile(t, (len(SWEEP), 1))
        block[:, k] = SWEEP
        rows.append(block)
    return np.concatenate(rows)


def tie_targets(T: int, low_pairs: bool = True) -> np.ndarray:
    """Rows placed by construction: all classes equal; two and three equal maxima at later classes;
    the saturation pairs in every pair of neighbouring classes (the others far below).
    ``low_pairs=False`` leaves out (-120, -100) and (-100, -120): under cloglog the oracle's own
    ``1 - exp(-e^eta)`` cancels to 0 below eta = -36.7 and ties there, which the cancellation-free
    reference does not; ``low_side_case`` pins those rows against the oracle itself."""
    rows = [np.full(T, v) for v in (0.0, 3.0, -2.5)]
    if T >= 2:
        for hi in (1.0, 40.0, -3.0):
            for i in range(T - 1):
                t = np.full(T, hi - 7.0)
                t[i] = t[i + 1] = hi
                rows.append(t)
            t = np.full(T, hi - 7.0)
            t[0] = t[T - 1] = hi
            rows.append(t)
        for a, b in PAIRS:
            if a < 0 and not low_pairs:
                continue
            for i in range(T - 1):
                t = np.full(T, min(a, b) - 50.0)
                t[i], t[i + 1] = a, b
                rows.append(t)
    return np.array(rows).reshape(-1, T)


def simplemax_targets(T: int) -> np.ndarray:
    """eta rows whose sum is a power of two (the division is exact: probabilities bit for bit), rows
    with sum 0 (no prediction), a negative sum, and equal maxima."""
    rows = []
    for total in (1.0, 2.0, 4.0, 8.0, 0.5, -2.0, -4.0, 0.0):
        for i in range(T):
            t = np.full(T, 0.25)
            t[i] = 1.5
            t[(i + 1) % T] += total - t.sum()
            rows.append(t)
        t = np.zeros(T)
        t[0] = t[T - 1] = total / 2 if T > 1 else total
        rows.append(t)
    rng = np.random.default_rng(5)
    rows += list(rng.integers(-16, 17, size=(64, T)) / 8.0)
    return np.array(rows).reshape(-1, T)


TARGET_SHAPES = {
    "clip-round": dict(min=-2.5, max=3.5, cast="round"),
    "clip-rescale-floor": dict(min=-0.75, max=1.25, factor=4.0, constant=1.0, cast="floor"),
    "rescale-ceiling": dict(factor=0.5, constant=0.25, cast="ceiling"),
    "round-default": dict(cast="round", default=-5.5),
    "clip-rescale": dict(min=-1.0, max=2.0, factor=-2.0, constant=0.5),
    "default-only": dict(default=7.0),
    "clip-rescale-round-default": dict(min=-2.0, max=2.0, factor=1.5, constant=0.0, cast="round", default=-9.0),
}


def target_values() -> np.ndarray:
    """Model values on +-k.5, on every clip bound of TARGET_SHAPES, on +-0.0 and around them."""
    v = list(np.arange(-40, 41) / 8.0) + [-0.0, 2.5, -2.5, 3.5, -3.5, 0.5, -0.5, 1.5, -1.5, 4.5, -4.5, -0.75, 1.25,
                                          -1.0, 2.0, -2.0, 100.0, -100.0]
    return np.array(v)


# --------------------------------------------------------------------------- the probe cases (CPU and GPU files)

SPECIAL_ETAS = (INF, -INF)


class Case:
    """One document with its probe rows: ``X`` fp32, ``eta`` / ``miss`` from the builder's arrays
    (guard asserted), ``special`` marks the rows that hold infinite or FLT_MAX cells on purpose."""

    def __init__(self, name: str, probe: Probe, X: np.ndarray, special: Optional[np.ndarray] = None):
        self.name, self.probe, self.X = name, probe, X
        self.special = np.zeros(len(X), bool) if special is None else special
        self.eta, self.miss = probe.eta(X, unguarded=self.special)
        for a in (self.X, self.eta, self.miss, self.special):
            a.setflags(write=False)

    def reference(self, fp32_rule: bool):
        p = self.probe
        return reference(self.eta, self.miss, p.K, p.norm, p.target, fp32_rule)

    def twin(self, mutant: str = ""):
        p = self.probe
        return twin_epilogue(self.eta, ~self.miss, p.K, p.norm, p.target, mutant=mutant)


def _thin(T: int) -> Sequence[int]:
    return range(T) if T <= 3 else (0, T // 2, T - 1)


def classification_case(K: int, F: int, norm: str, sparse: bool = False, zero_coef=None) -> Case:
    p = Probe(F, K, norm, sparse=sparse, zero_coef=zero_coef)
    name = f"K{K}-F{F}-{norm}" + ("-sparse" if sparse else "") + ("-zero" if zero_coef else "")
    if not p.steerable:  # few fields: the tables move together along field 0
        n = len(SWEEP)
        X = np.zeros((n, F))
        X[:, 0] = np.where(np.abs(SWEEP) <= 12, SWEEP, np.sign(SWEEP) * 12)
        X[:, 1:] = np.random.default_rng(F).integers(-8, 9, size=(n, F - 1)) / 8.0
        X[7::41, 0] = np.nan
        return Case(name, p, X.astype(F32))
    if norm == "simplemax":
        targets = simplemax_targets(K)
    else:
        sweep = sweep_targets(K)
        keep = np.concatenate([np.arange(k * len(SWEEP), (k + 1) * len(SWEEP)) for k in _thin(K)])
        targets = np.concatenate([sweep[keep], tie_targets(K, low_pairs=norm != "cloglog")])
    special = np.zeros(len(targets), bool)
    if sparse:  # a carrier at +-inf reaches its own table only: the other tables do not list it
        extra = []
        for k in _thin(K):
            for v in SPECIAL_ETAS:
                t = np.array([float(j % 3) - 1.0 for j in range(K)])
                t[k] = v
                extra.append(t)
        targets = np.concatenate([targets, np.array(extra)])
        special = np.concatenate([special, np.ones(len(extra), bool)])
    X = p.steer(targets, seed=K + F)
    special = np.concatenate([special, np.zeros(len(X) - len(special), bool)])  # the appended missing-cell rows
    return Case(name, p, X, special)


def low_side_case() -> Case:
    """cloglog, three tables, the low saturation pairs only (compare with the oracle, not the reference)."""
    p = Probe(6, 3, "cloglog")
    t = tie_targets(3)
    return Case("K3-F6-cloglog-low", p, p.steer(t[(t < -90).any(axis=1)], seed=1, nan_every=0))


# the largest fp32 eta and its five predecessors around ln(FLT_MAX): exp of the first is beyond
# FLT_MAX (the fp32 model-value rule), exp of the others is finite and must stay a prediction
_TOP = F32(88.7228394)
EXP_EDGE = tuple(float(_TOP - F32(k) * np.spacing(_TOP)) for k in range(6))


def regression_case(F: int, norm: str, target_name: Optional[str] = None) -> Case:
    """One regression table. Rows: the sweep (link ``none`` under a Target: ``target_values``), then
    eta = +-inf, one FLT_MAX cell (eta = FLT_MAX: still an fp32 number) and, from two fields on,
    FLT_MAX + FLT_MAX (finite in float64, an infinity in fp32)."""
    t = TARGET_SHAPES[target_name] if target_name else None
    p = Probe(F, 0, norm, target=t)
    base = target_values() if target_name else SWEEP
    X = p.steer(np.concatenate([base, SPECIAL_ETAS])[:, None], seed=F)
    if F == 1 and norm == "exp":  # one field: eta = -2 + x exactly, so these need no grid
        rows_edge = p.steer(np.array(EXP_EDGE)[:, None], nan_every=0)
    n_missing = len(X) - len(base) - 2
    rows = []
    for x0, xf in ((-FLT_MAX, 0.0), (FLT_MAX, 0.0), (-FLT_MAX, FLT_MAX), (FLT_MAX, -FLT_MAX)):
        r = np.zeros(F, F32)
        r[0] = x0
        if F > 1:
            r[1 + (COEFS[1:F].index(1.0) if 1.0 in COEFS[1:F] else 0)] = xf  # a filler with coefficient 1 (or -1)
        rows.append(r)
    X = np.concatenate([X, np.array(rows, F32)] + ([rows_edge] if F == 1 and norm == "exp" else []))
    special = np.zeros(len(X), bool)
    special[len(base):len(base) + 2] = True
    special[len(base) + 2 + n_missing:] = True
    return Case(f"reg-F{F}-{norm}" + (f"-{target_name}" if target_name else ""), p, X, special)


CLASS_NORMS = ("softmax", "simplemax") + LINKS
# (K, F, sparse): K = 1 is a single-table classifier (one class)
CLASS_SHAPES = ((1, 1, False), (1, 5, False), (2, 1, False), (2, 5, False), (3, 5, False), (3, 63, False), (16, 64, False), (3, 3, True),
                (2, 2, True), (16, 16, True))


def all_cases():
    """Every grid of the CPU file: every link x mode, K in {1, 2, 3, 16}, dense and sparse, the
    regression links and every Target shape. K = 1 is the degenerate classifier: an argmax over
    one class, validity from one link value, softmax 1 and simplemax eta / eta."""
    out = []
    for K, F, sparse in CLASS_SHAPES:
        for norm in CLASS_NORMS:
            if K == 16 and norm in ("probit", "cloglog", "loglog", "cauchit", "exp") and sparse:
                continue
            out.append(classification_case(K, F, norm, sparse))
    out.append(classification_case(3, 3, "logit", sparse=True, zero_coef=(1, 0)))
    for norm in LINKS:
        out.append(regression_case(5, norm))
    out.append(regression_case(1, "none"))
    out.append(regression_case(1, "exp"))
    for name in TARGET_SHAPES:
        out.append(regression_case(5, "none", name))
    out.append(regression_case(5, "exp", "clip-rescale-round-default"))
    return out


class GlmCase:
    """An ordinal or binomial ``GeneralRegressionModel`` over numeric covariates: ``eta [rows, K]``
    are the tables' linear predictors (the last ordinal / second binomial column is a placeholder),
    ``norm`` / ``labels`` what the dense lowering hands to linear.hip."""

    def __init__(self, kind: str, link: str, F: int, cuts: Sequence[float] = (), reference_first: bool = False):
        self.name = f"{kind}-{link}-F{F}" + ("-ref-first" if reference_first else "") \
            + ("".join(f"_{_num(c)}" for c in cuts))
        self.doc = glm_doc(kind, link, F, cuts, reference_first)
        shared = np.concatenate([SWEEP, [0.0, -20.0, -17.0, 20.0, 0.125, -0.125]])
        self.X, s = glm_inputs(shared, F, seed=F)
        self.miss = np.isnan(self.X).any(axis=1)
        if kind == "ordinal":
            self.K = len(cuts) + 1
            self.eta = np.concatenate([s[:, None] + np.asarray(cuts, np.float64)[None, :], np.zeros((len(s), 1))], axis=1)
            self.norm, self.labels = f"cumulative:{link}", class_labels(self.K)
        else:
            self.K = 2
            mirrored = {"logit": "logit", "probit": "probit", "cloglog": "loglog", "loglog": "cloglog"}
            glm = "none" if link == "identity" else link
            self.norm = mirrored[link] if reference_first else glm
            self.eta = np.stack([-s if reference_first else s, np.zeros(len(s))], axis=1)
            self.labels = class_labels(2) if reference_first else class_labels(2)[::-1]
        assert np.array_equal(self.eta.astype(F32).astype(np.float64), self.eta, equal_nan=True)
        self.eta = np.nan_to_num(self.eta)  # missing rows: validity comes from ``miss``

    def reference(self, fp32_rule: bool):
        return reference(self.eta, self.miss, self.K, self.norm, None, fp32_rule, self.labels)

    def twin(self, mutant: str = ""):
        return twin_epilogue(self.eta, ~self.miss, self.K, self.norm, labels=self.labels, mutant=mutant)


def glm_cases():
    """Ordinal cuts (0, 20): cumulative (0.5, saturated, 1) at a shared predictor of 0, and
    (2e-9, 0.5, 1) at -20, whose middle class ties with the last in fp32 only."""
    out = [GlmCase("ordinal", lk, 5, cuts) for lk in BOUNDED for cuts in ((0.0, 20.0), (-1.0, 1.125, 3.0))]
    out += [GlmCase("binomial", lk, 5) for lk in ("logit", "probit", "cloglog", "loglog", "identity")]
    out += [GlmCase("binomial", lk, 5, reference_first=True) for lk in ("logit", "cloglog")]
    return out


def oracle(c, X):
    """``(score, valid, probs or None)`` of the float64 oracle for a compiled document."""
    from flink_jpmml_amd.models.base import result_scores

    P, ok = c.prepare(np.asarray(X, np.float64))
    res, _ = c.evaluate_prepared(P)
    s, v = result_scores(res)
    v = v & ok
    return np.where(v, s, np.nan), v, getattr(res, "probs", None)


# |device - float64 reference| <= C 2^-24 (times the magnitude where the value leaves [0, 1]) per
# link, softmax and simplemax: 4 x the largest ratio measured on the MI355X against the float64
# reference, rounded up (docs/PARITY.md lists both numbers); none may exceed 16
MEASURED = {"logit": 2.03, "exp": 1.63, "probit": 1.28, "cloglog": 1.26, "loglog": 1.26, "cauchit": 1.34,
            "softmax": 2.28, "simplemax": 0.97}
C_BOUND = {k: 4 * v for k, v in MEASURED.items()}
C_BOUND["none"] = 0.0  # exact
assert max(C_BOUND.values()) <= 16


def magnitudes(K: int, norm: str, P: np.ndarray) -> np.ndarray:
    """What the rounding errors of ``P`` scale with: ``|P|`` itself, except under the two-table rule,
    where ``1 - p0`` inherits the absolute error of an unbounded ``p0`` (``exp`` of 1/16 is 1.0645:
    half an ulp of it is 15 x 2^-24 of the 0.0645 that is left)."""
    P = np.abs(np.asarray(P, np.float64))
    if K == 2 and norm in ("exp", "none"):
        return np.repeat(np.maximum(P[:, :1], P[:, 1:2]), 2, axis=1)
    return P


def value_bound(norm: str, ref: np.ndarray, C: Optional[float] = None) -> np.ndarray:
    """The bound on a probability / link value. Relative for ``exp`` and simplemax, whose values
    leave [0, 1]; below FLT_MIN fp32 keeps a spacing of 2^-149, not 24 bits, so the magnitude stops
    at FLT_MIN."""
    C = C_BOUND[norm] if C is None else C
    if norm in ("exp", "none", "simplemax"):
        return C * 2.0 ** -24 * np.maximum(np.abs(ref), FLT_MIN)
    return np.full(np.shape(ref), C * 2.0 ** -24)
