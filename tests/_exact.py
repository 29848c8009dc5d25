"""Exact-integer probes for the matrix-core kernels (gemm / mlp / svm / cluster / knn).

With small integer parameters and inputs every product and partial sum is an exact fp32 number
(and an exact bf16 operand), so the float64 oracle, a dense float64 reference and a correct kernel
agree in every bit, in any summation order. An index, padding, permutation, tail or tie error then
shows as a whole-integer difference instead of hiding inside a tolerance.

This module holds the document builders (caller-chosen parameters; ``bench/synth.py`` only draws
random ones), the input matrices, the dense float64 references computed from the builders' own
arrays, the exactness guard every probe asserts, and the named mutants of the packed tensors."""

import io
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from flink_jpmml_amd.bench.synth import _data_dictionary, _header, _mining_schema

F32 = np.float32


def bits(x) -> np.ndarray:
    """fp32 bit patterns (the comparison of every probe: ``np.array_equal`` on these)."""
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32)


def _num(v) -> str:
    v = float(v)
    return str(int(v)) if v == int(v) else repr(v)


# --------------------------------------------------------------------------- inputs


def probe_matrix(rows: int, n_features: int, seed: int, lo: int = -2, hi: int = 2, nan_every: int = 37,
                 density: float = 1.0, missing_rows: Sequence[int] = ()) -> np.ndarray:
    """fp32 ``[rows, F]`` of small integers: the all-zero row, the one-hot rows ``c e_j`` of every
    input j (c cycles through +-1, +-2; they come first so that a short batch still holds them),
    then uniform integers in ``lo..hi`` (only a share ``density`` of the cells, the others zero: small
    sums, so many land exactly on a threshold). Every ``nan_every``-th row from row 5 carries one NaN
    and the ``missing_rows`` are all NaN; the one-hot rows step over both, so every input keeps a
    valid one-hot row."""
    rng = np.random.default_rng(seed)
    X = rng.integers(lo, hi + 1, size=(rows, n_features)).astype(F32)
    if density < 1.0:
        X[rng.random(X.shape) >= density] = 0.0
    if rows > 1:
        X[0] = 0.0
    nan_rows = set(range(5, rows, nan_every)) if nan_every else set()
    cs = [1, -1, 2, -2]
    r = 1
    for j in range(n_features):
        while r in nan_rows or r in missing_rows:
            r += 1
        if r >= rows:
            break
        X[r] = 0.0
        X[r, j] = cs[(j + seed) % 4]
        r += 1
    for r in nan_rows:
        X[r, (7 * r) % n_features] = np.nan
    for r in missing_rows:
        if r < rows:
            X[r] = np.nan
    return X


def strided(X: np.ndarray, extra: int = 3) -> np.ndarray:
    """``X`` as a view of a wider matrix (row stride F + extra; the extra columns hold a value no
    model expects, so a kernel that ignores the stride reads it)."""
    wide = np.full((X.shape[0], X.shape[1] + extra), 97.0, dtype=F32)
    wide[:, : X.shape[1]] = X
    return wide


def assert_exact(values: Sequence[np.ndarray], bf16_values: Sequence[np.ndarray] = (), dyadic: float = 1.0) -> None:
    """The exactness guard. ``values`` (fp32 intermediates of the float64 reference): multiples of
    ``dyadic`` below 2**24 in magnitude; ``bf16_values`` (what a bf16 kernel rounds: inputs, hidden
    activations): integers of magnitude at most 256. A probe that fails here is a bad probe."""
    for v in values:
        v = np.asarray(v, np.float64)
        v = v[np.isfinite(v)]
        assert np.array_equal(np.round(v / dyadic) * dyadic, v), "intermediate is not an exact dyadic value"
        assert not v.size or np.abs(v).max() < 2 ** 24, float(np.abs(v).max())
    for v in bf16_values:
        v = np.asarray(v, np.float64)
        v = v[np.isfinite(v)]
        assert np.array_equal(np.round(v), v) and (not v.size or np.abs(v).max() <= 256), float(np.abs(v).max())


# --------------------------------------------------------------------------- neural networks

Layers = List[Tuple[np.ndarray, np.ndarray]]  # [(W[in, out], b[out])], integer valued float64


def int_network(n_in: int, hidden: Sequence[int], n_out: int, seed: int, taps: int = 3, wmax: int = 2,
                deep: bool = False, dups: Sequence[Tuple[int, int]] = ()) -> Layers:
    """Integer-weight network. Hidden unit u reads input ``(u + t m) % k`` for as many t as it takes
    the layer's m units to cover all k inputs, plus pseudo-random further inputs up to ``taps``,
    with weights from +-1..wmax and a bias from {-1, 0, 1} in the first layer; later layers read
    rectified values, so only their last tap may be negative (-1) and the bias is 0 or 1 (else units
    die on every row and hide their weights). ``deep``: two taps of 1 (the second sometimes -1) and
    an integer bias that keeps the unit active on about two of three random rows without letting
    its value double per layer, so eight layers stay inside bf16's exact integers and stay alive. Every output neuron is
    a checksum over ALL last-hidden units with position-dependent weights from +-{1, 2, 3} (a
    single-tap output would not notice a dropped column). ``dups``: output neuron ``dst`` copies
    ``src`` (equal logits on every row)."""
    rng = np.random.default_rng(seed)
    layers: Layers = []
    k = n_in
    # deep: the rows on which the biases centre the units (their own stream: the weights do not move)
    sample = np.random.default_rng(seed + 7919).integers(-2, 3, size=(512, n_in)).astype(np.float64)
    for li, m in enumerate(hidden):
        W = np.zeros((k, m))
        cover = -(-k // m)
        nt = 2 if deep else max(taps, cover + 1)
        nt = min(nt, k)
        for u in range(m):
            cols = [u % k] if deep else [(u + t * m) % k for t in range(cover)]
            while len(cols) < nt:
                c = int(rng.integers(k))
                if c not in cols:
                    cols.append(c)
            for t, c in enumerate(cols):
                w = int(rng.integers(1, (1 if deep else wmax) + 1))
                if li == 0 and not deep:
                    w = -w if rng.random() < 0.5 else w
                elif t == len(cols) - 1 and rng.random() < (0.15 if deep else 0.5):
                    w = -1  # rectified inputs: at most one negative tap, or the unit is dead on every row
                W[c, u] = w
        if deep:  # a unit is active on about two rows in three, and its value does not double per layer
            b = -np.floor(np.quantile(sample @ W, 0.35, axis=0))
            sample = np.maximum(sample @ W + b, 0.0)
        else:
            b = rng.integers(-1 if li == 0 else 0, 2, size=m).astype(np.float64)
        layers.append((W, b))
        k = m
    W = rng.integers(1, 4, size=(k, n_out)).astype(np.float64) * rng.choice([-1.0, 1.0], size=(k, n_out))
    for u in range(k):  # units 4, 16, 32, 64 or 256 apart never share a checksum weight: swapping them shows
        for o in range(n_out):
            while any(u >= d and W[u, o] == W[u - d, o] for d in (4, 16, 32, 64, 256)):
                W[u, o] = float(rng.integers(1, 4)) * float(rng.choice([-1.0, 1.0]))
    b = rng.integers(-2, 3, size=n_out).astype(np.float64)
    for src, dst in dups:
        W[:, dst], b[dst] = W[:, src], b[src]
    layers.append((W, b))
    return layers


def nn_pmml(layers: Layers, classification: bool = False, normalization: Optional[str] = "softmax",
            activations: Optional[Sequence[str]] = None, thresholds: Optional[Sequence[Optional[float]]] = None,
            net_threshold: Optional[float] = None, net_normalization: Optional[str] = None) -> str:
    """NeuralNetwork document of ``layers``: identity inputs (LinearNorm -1 -> -1, 1 -> 1), rectifier
    hidden layers, an identity output layer (``normalization`` for classification); only the
    non-zero connections are written. ``activations`` names every layer's ``activationFunction``
    instead (the network's stays rectifier), ``thresholds`` a ``threshold`` per layer (None: not
    written), ``net_threshold`` / ``net_normalization`` the NeuralNetwork element's own attributes
    (a layer without one inherits them). Weights and biases may then be dyadic fractions."""
    n_in, n_out = layers[0][0].shape[0], layers[-1][0].shape[1]
    out = io.StringIO()
    _header(out, "exact-integer network " + "-".join(str(W.shape[1]) for W, _ in layers))
    cats = [str(c) for c in range(n_out)] if classification else None
    _data_dictionary(out, n_in, "y", "integer" if classification else "double", cats)
    fn = "classification" if classification else "regression"
    net = "" if net_threshold is None else f' threshold="{_num(net_threshold)}"'
    net += f' normalizationMethod="{net_normalization}"' if net_normalization else ""
    out.write(f' <NeuralNetwork functionName="{fn}" activationFunction="rectifier"{net}>\n')
    _mining_schema(out, n_in, "y", "  ")
    out.write('  <NeuralInputs>\n')
    for j in range(n_in):
        out.write(f'   <NeuralInput id="i{j}"><DerivedField optype="continuous" dataType="double">'
                  f'<NormContinuous field="f{j}"><LinearNorm orig="-1" norm="-1"/><LinearNorm orig="1" norm="1"/>'
                  '</NormContinuous></DerivedField></NeuralInput>\n')
    out.write('  </NeuralInputs>\n')
    prev = [f"i{j}" for j in range(n_in)]
    for li, (W, b) in enumerate(layers):
        attrs = "" if activations is None else f' activationFunction="{activations[li]}"'
        if thresholds is not None and thresholds[li] is not None:
            attrs += f' threshold="{_num(thresholds[li])}"'
        if li == len(layers) - 1:
            if activations is None:
                attrs = ' activationFunction="identity"'
            if classification and normalization:
                attrs += f' normalizationMethod="{normalization}"'
        out.write(f'  <NeuralLayer{attrs}>\n')
        ids = []
        for u in range(W.shape[1]):
            ids.append(f"n{li}_{u}")
            out.write(f'   <Neuron id="{ids[-1]}" bias="{_num(b[u])}">')
            out.write("".join(f'<Con from="{prev[k]}" weight="{_num(W[k, u])}"/>' for k in np.flatnonzero(W[:, u])))
            out.write('</Neuron>\n')
        out.write('  </NeuralLayer>\n')
        prev = ids
    out.write('  <NeuralOutputs>\n')
    for k, nid in enumerate(prev):
        ex = f'<NormDiscrete field="y" value="{k}"/>' if classification else '<FieldRef field="y"/>'
        out.write(f'   <NeuralOutput outputNeuron="{nid}"><DerivedField optype="continuous" dataType="double">'
                  f'{ex}</DerivedField></NeuralOutput>\n')
    out.write('  </NeuralOutputs>\n </NeuralNetwork>\n</PMML>\n')
    return out.getvalue()


def nn_reference(layers: Layers, X: np.ndarray, classification: bool = False, guard: bool = True):
    """Dense float64 forward pass: ``(score, valid, logits)``; classification scores are the first
    maximum's class index. Asserts the exactness guard on its own intermediates."""
    X = np.asarray(X, np.float64)
    ok = ~np.isnan(X).any(axis=1)
    H = np.nan_to_num(X)
    seen, rounded = [], [H]
    for li, (W, b) in enumerate(layers):
        Z = H @ W + b
        seen.append(Z)
        if li < len(layers) - 1:
            H = np.maximum(Z, 0.0)
            rounded.append(H)
    if guard:
        assert_exact(seen, rounded)
    s = Z.argmax(axis=1).astype(np.float64) if classification else Z[:, 0]
    return np.where(ok, s, np.nan), ok, Z


def nn_insensitive(layers: Layers, X: np.ndarray) -> list:
    """Stored parameters (every non-zero weight ``(layer, k, unit)`` and every bias) whose change
    by +1 alters no compared output (the regression value / the integer logits) on any valid row
    of ``X``. Empty for a good probe: a dead unit or an unread column would hide an index error."""
    X = np.asarray(X, np.float64)
    X = X[~np.isnan(X).any(axis=1)]
    Hs, Zs = [X], []
    for li, (W, b) in enumerate(layers):
        Zs.append(Hs[-1] @ W + b)
        Hs.append(np.maximum(Zs[-1], 0.0))
    last = len(layers) - 1

    def shows(li, u, dz):
        if li == last:
            return bool(dz.any())
        dh = np.maximum(Zs[li][:, u] + dz, 0.0) - Hs[li + 1][:, u]
        rows = np.flatnonzero(dh)
        Wn = layers[li + 1][0][u]
        if not len(rows) or not Wn.any():
            return False
        if li + 1 == last:
            return True
        H = np.maximum(Zs[li + 1][rows] + dh[rows, None] * Wn[None, :], 0.0)
        for lj in range(li + 2, last + 1):
            Z = H @ layers[lj][0] + layers[lj][1]
            H = np.maximum(Z, 0.0)
        return not np.array_equal(Z, Zs[last][rows])

    missing = []
    ones = np.ones(len(X))
    for li, (W, b) in enumerate(layers):
        for u in range(W.shape[1]):
            if not shows(li, u, ones):
                missing.append((li, "bias", u))
            missing += [(li, int(k), u) for k in np.flatnonzero(W[:, u]) if not shows(li, u, Hs[li][:, k])]
    return missing


def nn_blind_positions(layers: Layers, X: np.ndarray) -> list:
    """Weight positions ``(layer, k, unit)``, stored or zero, that no valid row could show if a kernel
    filled them wrongly: input k of the layer is never non-zero on a row on which the unit is
    active (past its rectifier; an output neuron always is). Empty for a good probe."""
    X = np.asarray(X, np.float64)
    H = X[~np.isnan(X).any(axis=1)]
    blind = []
    for li, (W, b) in enumerate(layers):
        Z = H @ W + b
        active = np.ones_like(Z) if li == len(layers) - 1 else (Z > 0).astype(np.float64)
        seen = (H != 0).astype(np.float64).T @ active  # [k, unit]: rows with input k set and the unit active
        blind += [(li, int(k), int(u)) for k, u in zip(*np.nonzero(seen == 0))]
        H = np.maximum(Z, 0.0)
    return blind


def tie_rows(logits: np.ndarray) -> np.ndarray:
    """Rows whose maximum logit is reached by more than one class."""
    return (logits == logits.max(axis=1, keepdims=True)).sum(axis=1) > 1


# --------------------------------------------------------------------------- support vector machines


class SvmProbe:
    """Integer support vectors ``S [n_sv, F]`` and, per machine, the ids of its support vectors,
    their dual coefficients (+-{1, 2, 3}) and its intercept. ``n_classes`` 0: one regression
    machine; 2: one binary machine; more: one-against-one, every support vector owned by one class
    and used by the machines of that class."""

    def __init__(self, n_features: int, n_sv: int, n_classes: int, seed: int, kernel: str = "linear",
                 gamma: float = 0.125, lo: int = -2, hi: int = 2):
        rng = np.random.default_rng(seed)
        self.F, self.n_sv, self.n_classes, self.kernel, self.gamma = n_features, n_sv, n_classes, kernel, gamma
        self.S = rng.integers(lo, hi + 1, size=(n_sv, n_features)).astype(np.float64)
        pairs = [(a, b) for a in range(n_classes) for b in range(a + 1, n_classes)] if n_classes > 2 else [(0, 1)]
        owner = np.arange(n_sv) % max(n_classes, 1)
        rng.shuffle(owner)
        self.machines = []
        for a, b in pairs:
            ids = np.arange(n_sv) if n_classes <= 2 else np.flatnonzero((owner == a) | (owner == b))
            if not len(ids):
                ids = np.array([int(rng.integers(n_sv))])
            coef = rng.integers(1, 4, size=len(ids)) * rng.choice([-1, 1], size=len(ids))
            # the intercept is a multiple of a coefficient: decision values land exactly on the threshold 0
            self.machines.append((ids, coef.astype(np.float64), float(coef[0] * rng.integers(-1, 2)), a, b))
        M = len(self.machines)
        self.A = np.zeros((n_sv, M))
        self.b = np.zeros(M)
        for m, (ids, coef, b0, _, _) in enumerate(self.machines):
            self.A[ids, m] = coef
            self.b[m] = b0

    def pmml(self) -> str:
        out = io.StringIO()
        _header(out, f"exact-integer SVM {self.kernel}")
        cls = self.n_classes >= 2
        cats = [str(c) for c in range(self.n_classes)] if cls else None
        _data_dictionary(out, self.F, "y", "integer" if cls else "double", cats)
        ovo = ' classificationMethod="OneAgainstOne"' if self.n_classes > 2 else ""
        out.write(f' <SupportVectorMachineModel functionName="{"classification" if cls else "regression"}" '
                  f'svmRepresentation="SupportVectors"{ovo}>\n')
        _mining_schema(out, self.F, "y", "  ")
        g = repr(self.gamma)
        out.write("  " + {"linear": '<LinearKernelType/>', "radialBasis": f'<RadialBasisKernelType gamma="{g}"/>',
                          "polynomial": f'<PolynomialKernelType gamma="{g}" coef0="1" degree="3"/>',
                          "sigmoid": f'<SigmoidKernelType gamma="{g}" coef0="0.5"/>'}[self.kernel] + "\n")
        out.write(f'  <VectorDictionary numberOfVectors="{self.n_sv}">\n   <VectorFields numberOfFields="{self.F}">')
        out.write("".join(f'<FieldRef field="f{j}"/>' for j in range(self.F)) + '</VectorFields>\n')
        for i in range(self.n_sv):
            out.write(f'   <VectorInstance id="sv{i}"><Array n="{self.F}" type="real">'
                      + " ".join(_num(v) for v in self.S[i]) + '</Array></VectorInstance>\n')
        out.write('  </VectorDictionary>\n')
        for ids, coef, b0, a, b in self.machines:
            tc = f' targetCategory="{a}" alternateTargetCategory="{b}"' if cls else ""
            out.write(f'  <SupportVectorMachine{tc}>\n   <SupportVectors numberOfSupportVectors="{len(ids)}">')
            out.write("".join(f'<SupportVector vectorId="sv{i}"/>' for i in ids) + '</SupportVectors>\n')
            out.write(f'   <Coefficients numberOfCoefficients="{len(ids)}" absoluteValue="{_num(b0)}">')
            out.write("".join(f'<Coefficient value="{_num(c)}"/>' for c in coef))
            out.write('</Coefficients>\n  </SupportVectorMachine>\n')
        out.write(' </SupportVectorMachineModel>\n</PMML>\n')
        return out.getvalue()

    def reference(self, X: np.ndarray, guard: bool = True):
        """Linear kernel, dense float64: ``(score, valid, decision [rows, machines])``; votes as the
        specification (D < 0: the machine's first class), ties to the first category."""
        assert self.kernel == "linear"
        X = np.asarray(X, np.float64)
        ok = ~np.isnan(X).any(axis=1)
        G = np.nan_to_num(X) @ self.S.T
        D = G @ self.A + self.b
        if guard:
            assert_exact([G, D, np.abs(G) @ np.abs(self.A)])
        if self.n_classes < 2:
            s = D[:, 0]
        else:
            votes = np.zeros((len(X), self.n_classes))
            for m, (_, _, _, a, b) in enumerate(self.machines):
                first = D[:, m] < 0
                votes[first, a] += 1
                votes[~first, b] += 1
            s = votes.argmax(axis=1).astype(np.float64)
        return np.where(ok, s, np.nan), ok, D

    def kernel_terms(self, X: np.ndarray):
        """Polynomial / RBF / sigmoid: float64 ``(D, T)`` with ``T[r, m] = sum_j |a_jm| |K_j| (1 + |arg_j|)
        + |D|``, the magnitude an fp32 evaluation's rounding errors scale with (``arg`` is what the
        kernel function is applied to: gamma x.s + coef0, or gamma |x - s|^2)."""
        X = np.nan_to_num(np.asarray(X, np.float64))
        G = X @ self.S.T
        if self.kernel == "radialBasis":
            arg = self.gamma * np.maximum((X * X).sum(1)[:, None] - 2.0 * G + (self.S * self.S).sum(1)[None], 0.0)
            K = np.exp(-arg)
        elif self.kernel == "polynomial":
            arg = self.gamma * G + 1.0
            K = arg ** 3
        else:
            arg = self.gamma * G + 0.5
            K = np.tanh(arg)
        D = K @ self.A + self.b
        return D, (np.abs(K) * (1.0 + np.abs(arg))) @ np.abs(self.A) + np.abs(D)


# --------------------------------------------------------------------------- clustering / k-NN


def grid_range(K: int, n_features: int, lo: int = -3, hi: int = 3) -> Tuple[int, int]:
    """``lo..hi`` widened until the grid holds at least 4 K points (few fields: else every centre has twins)."""
    while (hi - lo + 1) ** n_features < 4 * K:
        lo, hi = 2 * lo, 2 * hi
    return lo, hi


def grid_centers(K: int, n_features: int, seed: int, lo: int = -3, hi: int = 3) -> np.ndarray:
    """Distinct integer centres, then duplicates at k + 4 (the other lane half of a 32-wide tile)
    and k + 32 (the next tile) of every 7th centre: exact ties whose winner is the lower index."""
    rng = np.random.default_rng(seed)
    lo, hi = grid_range(K, n_features, lo, hi)
    seen, rows = set(), []
    while len(rows) < K:
        c = tuple(int(v) for v in rng.integers(lo, hi + 1, size=n_features))
        if c not in seen:
            seen.add(c)
            rows.append(c)
    C = np.array(rows, dtype=np.float64)
    for k in range(0, K, 7):
        for d in (4, 32):
            if k + d < K and (k + d) % 7:
                C[k + d] = C[k]
    return C


def shadowed(C: np.ndarray) -> List[int]:
    """Centres that repeat an earlier one (they never win a tie)."""
    first = {}
    return [k for k, c in enumerate(map(tuple, C)) if first.setdefault(c, k) != k]


def center_matrix(C: np.ndarray, rows: int, seed: int, nan_every: int = 11) -> np.ndarray:
    """Probe rows for centres ``C``: ``rows`` grid rows (zero row, one-hot rows, uniform integers over
    the centres' range, a NaN in every ``nan_every``-th, row 16 all missing), then every centre
    itself and, for every shadowed centre and field, that centre moved one step along the field
    (where the shadowed centre, moved the same way, would win alone)."""
    K, Fn = C.shape
    lo, hi = grid_range(K, Fn)
    X = probe_matrix(rows, Fn, seed=seed, lo=lo, hi=hi, nan_every=nan_every, missing_rows=(16,))
    extra = [C] + [C[k][None, :] + np.eye(Fn) for k in shadowed(C)]
    return np.concatenate([X] + extra).astype(F32)


def centers_insensitive(C: np.ndarray, w: np.ndarray, X: np.ndarray) -> list:
    """Centre entries ``(k, f)`` whose change by +1 alters neither the label nor the (squared
    Euclidean) affinity of any complete row of ``X``. Empty for a good probe."""
    X = np.asarray(X, np.float64)
    X = X[~np.isnan(X).any(axis=1)]
    raw = raw_distances(C, w, X, "squaredEuclidean")
    label = raw.argmin(axis=1)
    best = raw[np.arange(len(X)), label]
    missing = []
    for k in range(len(C)):
        new = raw[:, [k]] + w[None, :] * (1.0 - 2.0 * (X - C[k][None, :]))  # [rows, F]: entry f moved by +1
        mine = (label == k)[:, None]
        other = np.where(np.arange(len(C))[None, :] == k, np.inf, raw)
        ob = other.min(axis=1)[:, None]
        ok_ = other.argmin(axis=1)[:, None]
        changed = np.where(mine, (new != best[:, None]) | (new > ob) | ((new == ob) & (ok_ < k)),
                           (new < best[:, None]) | ((new == best[:, None]) & (k < label[:, None])))
        missing += [(k, int(f)) for f in np.flatnonzero(~changed.any(axis=0))]
    return missing


def field_weights(n_features: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed + 1000).choice([0.5, 1.0, 2.0], size=n_features)


def cluster_pmml(C: np.ndarray, w: np.ndarray, metric: str) -> str:
    K, Fn = C.shape
    out = io.StringIO()
    _header(out, f"exact-integer clustering {K} x {Fn}")
    out.write(f' <DataDictionary numberOfFields="{Fn + 1}">\n')
    for j in range(Fn):
        out.write(f'  <DataField name="f{j}" optype="continuous" dataType="float"/>\n')
    out.write('  <DataField name="cluster" optype="categorical" dataType="string"/>\n </DataDictionary>\n')
    out.write(f' <ClusteringModel modelName="probe" functionName="clustering" modelClass="centerBased" '
              f'numberOfClusters="{K}">\n  <MiningSchema>\n   <MiningField name="cluster" usageType="predicted"/>\n')
    for j in range(Fn):
        out.write(f'   <MiningField name="f{j}"/>\n')
    out.write(f'  </MiningSchema>\n  <ComparisonMeasure kind="distance"><{metric}/></ComparisonMeasure>\n')
    for j in range(Fn):
        out.write(f'  <ClusteringField field="f{j}" compareFunction="absDiff" fieldWeight="{_num(w[j])}"/>\n')
    for k in range(K):
        out.write(f'  <Cluster id="{k + 1}" name="c{k + 1}"><Array n="{Fn}" type="real">'
                  + " ".join(_num(v) for v in C[k]) + '</Array></Cluster>\n')
    out.write(' </ClusteringModel>\n</PMML>\n')
    return out.getvalue()


def raw_distances(C: np.ndarray, w: np.ndarray, X: np.ndarray, metric: str) -> np.ndarray:
    """Dense float64 ``[rows, K]`` raw sums over the present fields (before the missing-value
    rescale and the root): exact multiples of 0.5 for integer data and weights from {0.5, 1, 2}."""
    X = np.asarray(X, np.float64)
    pres = ~np.isnan(X)
    Xz = np.nan_to_num(X)
    if metric in ("squaredEuclidean", "euclidean"):
        # sum w (x - c)^2 over present fields, as three exact products
        return (pres * w * Xz * Xz).sum(1)[:, None] - 2.0 * (Xz * w) @ C.T + (pres * w) @ (C * C).T
    d = np.abs(Xz[:, None, :] - C[None]) * w * pres[:, None, :]
    return d.sum(-1) if metric == "cityBlock" else d.max(-1)


def cluster_reference(C: np.ndarray, w: np.ndarray, X: np.ndarray, metric: str, guard: bool = True):
    """``(label (first minimum), affinity float64, valid, raw [rows, K])``; complete rows' affinity
    is exact (its root rounded once for euclidean), rows with a missing field carry the rescale."""
    raw = raw_distances(C, w, X, metric)
    if guard:
        assert_exact([raw], dyadic=0.5)
    pres = ~np.isnan(np.asarray(X, np.float64))
    label = raw.argmin(axis=1)
    best = raw[np.arange(len(raw)), label]
    if metric != "chebychev":
        with np.errstate(divide="ignore", invalid="ignore"):
            best = best * (X.shape[1] / pres.sum(1))
    if metric == "euclidean":
        best = np.sqrt(best)
    return label, best, pres.any(axis=1), raw


def min_tie_rows(raw: np.ndarray) -> np.ndarray:
    return (raw == raw.min(axis=1, keepdims=True)).sum(axis=1) > 1


def knn_pmml_exact(inst: np.ndarray, targets: Sequence, k: int, method: str, metric: str = "squaredEuclidean",
                   classes: int = 0) -> str:
    N, Fn = inst.shape
    out = io.StringIO()
    _header(out, f"exact-integer {k}-NN")
    cats = [str(c) for c in range(classes)] if classes else None
    _data_dictionary(out, Fn, "y", "string" if classes else "double", cats)
    fn = "classification" if classes else "regression"
    meth = f' categoricalScoringMethod="{method}"' if classes else f' continuousScoringMethod="{method}"'
    out.write(f' <NearestNeighborModel functionName="{fn}" numberOfNeighbors="{k}"{meth}>\n')
    _mining_schema(out, Fn, "y", "  ")
    out.write(f'  <TrainingInstances recordCount="{N}" fieldCount="{Fn + 1}">\n   <InstanceFields>')
    out.write("".join(f'<InstanceField field="f{j}" column="c{j}"/>' for j in range(Fn)))
    out.write('<InstanceField field="y" column="target"/></InstanceFields>\n   <InlineTable>\n')
    for i in range(N):
        out.write("    <row>" + "".join(f"<c{j}>{_num(inst[i, j])}</c{j}>" for j in range(Fn))
                  + f"<target>{_num(targets[i])}</target></row>\n")
    out.write('   </InlineTable>\n  </TrainingInstances>\n')
    out.write(f'  <ComparisonMeasure kind="distance"><{metric}/></ComparisonMeasure>\n  <KNNInputs>')
    out.write("".join(f'<KNNInput field="f{j}"/>' for j in range(Fn)))
    out.write('</KNNInputs>\n </NearestNeighborModel>\n</PMML>\n')
    return out.getvalue()


def knn_reference(inst: np.ndarray, targets: np.ndarray, X: np.ndarray, k: int, method: str, metric: str,
                  guard: bool = True):
    """``(score, valid, kth_tie)``: the k nearest by (raw sum, index) — the rescale and the root are
    monotone per row — aggregated; ``kth_tie`` marks rows whose k-th and (k+1)-th neighbours are
    equidistant (the lower index must win)."""
    raw = raw_distances(inst, np.ones(inst.shape[1]), X, metric)
    if guard:
        assert_exact([raw])
    order = np.argsort(raw, axis=1, kind="stable")
    rs = np.take_along_axis(raw, order, axis=1)
    tie = rs[:, k - 1] == rs[:, k] if raw.shape[1] > k else np.zeros(len(raw), bool)
    y = np.asarray(targets)[order[:, :k]]
    if method == "majorityVote":
        s = np.empty(len(raw))
        for r in range(len(raw)):  # most votes; among equals the class whose best member ranks first
            vals, first, cnt = np.unique(y[r], return_index=True, return_counts=True)
            top = cnt == cnt.max()
            s[r] = vals[top][np.argmin(first[top])]
    elif method == "median":
        s = np.median(y, axis=1)
    else:
        s = y.sum(axis=1) / k
    ok = ~np.isnan(np.asarray(X, np.float64)).all(axis=1)
    return np.where(ok, s, np.nan), ok, tie


# --------------------------------------------------------------------------- mutants of packed tensors


def _swap(a: np.ndarray, axis: int, i: int, j: int) -> None:
    idx_i, idx_j = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    idx_i[axis], idx_j[axis] = i, j
    tmp = a[tuple(idx_i)].copy()
    a[tuple(idx_i)] = a[tuple(idx_j)]
    a[tuple(idx_j)] = tmp


def layer_mutants(k: int, m: int) -> Dict[str, callable]:
    """Named mutants of one layer given as its padded ``Wt [units, k]`` and ``bias [units]`` (modified
    in place); ``k`` / ``m`` are the layer's real input / unit counts. A mutant the layer cannot hold
    (no unit 32 / 256 further, no column 16 / 64 further) is left out."""
    def zero_col(Wt, b):
        Wt[:, k - 1] = 0

    def zero_unit(Wt, b):
        Wt[m - 1, :] = 0
        b[m - 1] = 0

    def swap_units(d):
        def f(Wt, b):
            _swap(Wt, 0, m - 1 - d, m - 1)
            _swap(b, 0, m - 1 - d, m - 1)
        return f

    def swap_cols(d):
        def f(Wt, b):
            _swap(Wt, 1, 0, d)
        return f

    def bias(d):
        def f(Wt, b):
            b[m - 1] += d
        return f

    out = {"zero-last-k-column": zero_col, "zero-last-unit": zero_unit, "bias+1-last-unit": bias(1.0),
           "bias-1-last-unit": bias(-1.0)}
    if m > 32:
        out["swap-units-32-apart"] = swap_units(32)
    if m > 256:
        out["swap-units-across-256-block"] = swap_units(256)
    if k > 16:
        out["swap-k-columns-16-apart"] = swap_cols(16)
    if k > 64:
        out["swap-k-columns-64-apart"] = swap_cols(64)
    return out


def wide_mutants(dims, n_in: int, layers: Layers) -> Dict[str, callable]:
    """``layer_mutants`` of the first layer on a ``WideMlpPlan``'s packed ``(wts, bss)`` (float
    arrays, modified in place). Each must change at least one compared bit of the probe's outputs."""
    kp, mp, _, _, wo, bo = dims[0]
    k, m = layers[0][0].shape  # real sizes of the first layer

    def on_packed(f):
        return lambda W, B: f(W[wo: wo + mp * kp].reshape(mp, kp), B[bo: bo + mp])

    return {name: on_packed(f) for name, f in layer_mutants(k, m).items()}


# --------------------------------------------------------------------------- the probe cases (CPU and GPU files)

# fused MLP (mlp.hip): name -> int_network arguments + classification
FUSED_SHAPES = {
    "17-33-1": dict(n_in=17, hidden=(33,), n_out=1),
    "21-50-33-7cls": dict(n_in=21, hidden=(50, 33), n_out=7, dups=((1, 5),)),
    "64-256-256-1": dict(n_in=64, hidden=(256, 256), n_out=1),
    "255-31-1": dict(n_in=255, hidden=(31,), n_out=1),
    "16-32x7-1": dict(n_in=16, hidden=(32,) * 7, n_out=1, deep=True),
    "12-40-32cls": dict(n_in=12, hidden=(40,), n_out=32, dups=((2, 21), (7, 8))),
}

# wide MLP (gemm.hip)
WIDE_SHAPES = {
    "33-300-1": dict(n_in=33, hidden=(300,), n_out=1),
    "65-257-300-1": dict(n_in=65, hidden=(257, 300), n_out=1),
    "600-1024-1": dict(n_in=600, hidden=(1024,), n_out=1),
    "64-512-1": dict(n_in=64, hidden=(512,), n_out=1),
    "1030-257-1": dict(n_in=1030, hidden=(257,), n_out=1),
    "40-300-1024-1": dict(n_in=40, hidden=(300, 1024), n_out=1),
    "8-300-33cls": dict(n_in=8, hidden=(300,), n_out=33, dups=((0, 32), (3, 20))),
    "8-300-40cls": dict(n_in=8, hidden=(300,), n_out=40, dups=((5, 37),)),
    "24-512-768-4cls": dict(n_in=24, hidden=(512, 768), n_out=4, dups=((0, 3),)),
}
# Two models with different position patterns per shape. A stored parameter can still hide (a unit
# that is dead on every row, two checksum weights that cancel a shared change), so the seeds are the
# first two for which nn_insensitive() and nn_blind_positions() are empty; tests/test_exact_probes.py asserts
# that they are.
_SEEDS = {"64-256-256-1": (3, 9), "16-32x7-1": (2, 3), "65-257-300-1": (11, 14)}


def seeds(name: str) -> Tuple[int, int]:
    return _SEEDS.get(name, (1, 2))


def network(shape: dict, seed: int, norm: Optional[str] = "softmax"):
    """``(layers, classification, document)`` of a FUSED_SHAPES / WIDE_SHAPES entry. ``norm=None``
    leaves the output layer un-normalised: the class probabilities a plan writes are then the
    integer logits themselves and compare bit for bit (labels alone are too coarse to see every
    weight), so every classification shape runs with softmax and without."""
    layers = int_network(seed=seed, **shape)
    cls = shape["n_out"] > 1
    return layers, cls, nn_pmml(layers, cls, norm)


def norms(shape: dict):
    return ("softmax", None) if shape["n_out"] > 1 else ("softmax",)


def nn_rows(n_in: int) -> int:
    """Rows of a network probe: the zero row, every one-hot row and at least 500 dense rows."""
    return max(769, n_in + n_in // 37 + 502)


ROW_COUNTS = (1, 33, 129, 257)

# SVM (svm.hip): name -> (features, support vectors, classes, plan class name)
SVM_ROWS = 513
SVM_CASES = {
    "valu-1sv": (8, 1, 2, "SvmPlan"), "valu-31sv": (9, 31, 3, "SvmPlan"),
    "mfma-32sv": (8, 32, 2, "SvmPlan"), "mfma-33sv": (9, 33, 3, "SvmPlan"), "mfma-65sv": (64, 65, 4, "SvmPlan"),
    "mfma-reg": (9, 33, 0, "SvmPlan"),
    "wide-5cls": (16, 31, 5, "SvmWidePlan"), "wide-9cls": (17, 33, 9, "SvmWidePlan"),
    "wide-12cls": (65, 64, 12, "SvmWidePlan"), "wide-17cls": (128, 64, 17, "SvmWidePlan"),
    "wide-1sv": (16, 1, 5, "SvmWidePlan"), "wide-reg-f100": (100, 33, 0, "SvmWidePlan"),
}
NONLINEAR_SVM_CASES = ("valu-31sv", "mfma-33sv", "mfma-65sv", "wide-9cls", "wide-12cls", "wide-reg-f100")
# polynomial / RBF / sigmoid SVM decisions: 4 x the largest |device - oracle| / (2^-24 T) measured on
# the MI355X (1.648; T: SvmProbe.kernel_terms), which leaves room for another summation order
SVM_ULP_CONSTANT = 4 * 1.65


def svm_probe(name: str, seed: int = 3, kernel: str = "linear"):
    """``(SvmProbe, plan class name)`` of an SVM_CASES entry."""
    F, nsv, C, kind = SVM_CASES[name]
    gamma = 2.0 ** -int(np.ceil(np.log2(4 * F)))  # a power of two near 1 / (4 F): kernel arguments of order 1
    return SvmProbe(F, nsv, C, seed=seed + nsv, kernel=kernel, gamma=gamma), kind


CLUSTER_CASES = [(31, 1), (32, 7), (33, 33), (100, 128)]  # (K, F)

KNN_CASES = [
    # (instances, k, method, metric, features)
    (2, 2, "majorityVote", "squaredEuclidean", 3), (33, 8, "majorityVote", "euclidean", 2),
    (65, 9, "median", "squaredEuclidean", 3), (300, 32, "average", "euclidean", 4),
    (300, 9, "majorityVote", "squaredEuclidean", 3), (65, 2, "average", "squaredEuclidean", 5),
    (33, 3, "median", "euclidean", 2), (32, 32, "majorityVote", "squaredEuclidean", 2),
]


def knn_probe(N: int, k: int, method: str, metric: str, F: int):
    """``(instances, targets, classes)``: grid instances with duplicates, class ids or integer values."""
    inst = grid_centers(N, F, seed=N + k)
    rng = np.random.default_rng(N * 31 + k)
    classes = 3 if method == "majorityVote" else 0
    targets = rng.integers(0, 3, N) if classes else rng.integers(-8, 9, N)
    return inst, targets.astype(np.float64), classes


def svm_matrix(rows: int, n_features: int, seed: int = 5) -> np.ndarray:
    """Sparse -1 / 0 / 1 rows: decision values are small integers and many are exactly 0."""
    return probe_matrix(rows, n_features, seed=seed, lo=-1, hi=1, density=min(1.0, 4.0 / n_features))
