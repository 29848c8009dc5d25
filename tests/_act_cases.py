"""Activation and output-normalisation probes for the network kernels (mlp.hip, gemm.hip).

The exact-integer probes of ``tests/_exact.py`` are rectifier networks with an identity output
layer. Here the activation is the only rounded step: every layer is the identity except one layer
under test, all weights up to it are integers of magnitude at most 4 and the inputs are ``m / 16``
with ``|m| <= 64``, so unit j of the tested layer has the pre-activation ``z_j = a_j x + b_j``, an
exact fp32 number (and an exact bf16 operand chain) known in closed form. Everything after the
tested layer is a one-hot tap of weight 1 and bias 0, so an output equals ``f(z)`` of the unit it
reads: exactly in fp32, rounded once to bf16 where a bf16 kernel carries a hidden activation.

This module holds the builders, the input batches, the float64 reference
(``models.neural.activate`` on the exact z), the comparison rules (bit for bit, or a scaled bound
whose constants were measured on the MI355X), the numpy twin of the device formulas with its
named mutants, and the registry of kernel paths that the CPU and the GPU file both walk."""

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import _exact as E
from flink_jpmml_amd.models.neural import activate, normalize_layer

F32 = np.float32
U = 2.0 ** -24  # half an fp32 ulp of 1: the unit of every scaled bound

ACTS = ("identity", "logistic", "tanh", "rectifier", "exponential", "reciprocal", "square", "Gauss", "sine",
        "cosine", "Elliott", "arctan", "threshold")
# compared with np.array_equal on the bit patterns: no rounded step but one correctly rounded
# division (reciprocal, Elliott: numerator and denominator exact, integers below 2^12 after scaling)
EXACT_ACTS = ("identity", "rectifier", "square", "threshold", "reciprocal", "Elliott")
THR = 0.25  # the threshold under test; NET_THR is what the network declares when the layer sets THR
NET_THR = 1.0

# (label, activation, layer threshold, network threshold)
VARIANTS = [(a, a, None, None) for a in ACTS if a != "threshold"] + [
    ("threshold@layer", "threshold", THR, NET_THR), ("threshold@network", "threshold", None, THR)]

# Domain of the pre-activations, per function: every z of a compared entry is a multiple of 1/16
# (1/32 off it for reciprocal) with |z| <= 16; the bounded functions hold their bound on all of
# it, Gauss and logistic through the underflow floor TINY where f(z) leaves fp32's normal range.
DOMAIN = {a: 16.0 for a in ACTS}
DOMAIN["reciprocal"] = 16.0 + 1.0 / 32
POLE_SHIFT = 1.0 / 32  # reciprocal: every bias is moved off the grid, so no unit (read or not) sits on z = 0
TINY = 2.0 ** -102  # U * TINY = 2^-126, the smallest normal fp32: __expf flushes below it

# ---- measured on the MI355X: largest |device - ref64| / (U S_f(z)) over every site, kernel and case
# of tests/test_gpu_activations.py (docs/PARITY.md holds the per-site table). C_f = 4 x that.
MEASURED_RATIO = {"logistic": 14.47, "tanh": 1.32, "exponential": 1.08, "Gauss": 0.95, "sine": 22.41,
                  "cosine": 14.80, "arctan": 2.15}
C = {a: 4.0 * r for a, r in MEASURED_RATIO.items()}
SOFTMAX_MEASURED_RATIO = 0.99
SOFTMAX_C = 4.0 * SOFTMAX_MEASURED_RATIO


def bf16_rn(x) -> np.ndarray:
    """fp32 -> nearest bf16 (ties to even), returned as fp32."""
    b = E.bits(x).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def is_bf16(x) -> np.ndarray:
    return (E.bits(x) & 0xFFFF) == 0


def half_bf16_ulp(x) -> np.ndarray:
    """Half the spacing of bf16 numbers at |x| (float64): 2^(e - 9) for 2^(e-1) <= |x| < 2^e."""
    _, e = np.frexp(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126))
    return np.ldexp(1.0, e - 9)


def scale(act: str, z: np.ndarray, f: np.ndarray) -> np.ndarray:
    """S_f(z) of the scaled bound, from the float64 reference alone."""
    f = np.abs(f)
    if act == "exponential":
        return np.maximum(f * (1.0 + np.abs(z)), TINY)
    if act == "Gauss":
        return np.maximum(f * (1.0 + z * z), TINY)
    if act in ("sine", "cosine"):
        return np.ones_like(f)  # __sinf / __cosf are absolute, not relative, near their zeros
    return np.maximum(f, TINY)


def bound(act: str, z: np.ndarray, f: np.ndarray, bf16_rounded: bool) -> np.ndarray:
    b = C[act] * U * scale(act, z, f)
    return b + half_bf16_ulp(f) if bf16_rounded else b


# --------------------------------------------------------------------------- ramp networks

# distinct (a, b) with 4 |a| + |b| <= 16; the first entries are the ones a single output reads
AB = [(4, 0), (1, 0), (-4, 0), (-1, 0), (2, 0), (-2, 0), (3, 0), (-3, 0)]
AB += [(a, b) for a in (3, -3) for b in (-4, -1, 1, 4)] + [(a, b) for a in (2, -2) for b in (-8, -3, 3, 8)]
AB += [(a, b) for a in (1, -1) for b in (-12, -8, -4, -1, 1, 4, 8, 12)]
assert len(set(AB)) == len(AB) and all(4 * abs(a) + abs(b) <= 16 for a, b in AB)


class Ramp:
    """One network: layer sizes ``hidden + (n_out,)``, layer ``tested`` carries ``act`` (the last
    index: the output site), every other layer the identity (``post_act``: the output layer's
    activation when a hidden layer is tested; the two-site cases).

    Layers before the tested one: unit u reads unit ``u % k`` of the layer below with weight 1.
    Tested layer: unit u reads unit ``(5 u + seed) % k`` with weight ``a_u`` and has bias ``b_u``,
    ``(a_u, b_u) = AB[(u - sel0 + seed) % len(AB)]`` where sel0 is the unit the first output reads, so
    a one-output network probes AB[seed]. Layers after it: one tap of weight 1, bias 0."""

    def __init__(self, n_in: int, hidden: Sequence[int], n_out: int, tested: int, act: str, seed: int,
                 layer_thr: Optional[float] = None, net_thr: Optional[float] = None, post_act: str = "identity",
                 pole_shift: Optional[float] = None, ab: Optional[Sequence[Tuple[float, float]]] = None):
        sizes = list(hidden) + [n_out]
        L = len(sizes)
        assert 0 <= tested < L
        self.n_in, self.sizes, self.n_out, self.tested, self.act, self.seed = n_in, sizes, n_out, tested, act, seed
        self.layer_thr, self.net_thr, self.post_act = layer_thr, net_thr, post_act
        self.thr = layer_thr if layer_thr is not None else (net_thr if net_thr is not None else 0.0)
        # wiring after the tested layer: src[li][u] = the unit of layer li - 1 that unit u reads
        self.src: Dict[int, np.ndarray] = {}
        for li in range(tested + 1, L):
            k = sizes[li - 1]
            step = 7 if li == L - 1 else 1
            self.src[li] = (step * np.arange(sizes[li]) + 3 * li + seed) % k
        sel = np.arange(n_out)
        for li in range(L - 1, tested, -1):
            sel = self.src[li][sel]
        self.sel = sel  # tested-layer unit behind every output
        m, k = sizes[tested], (n_in if tested == 0 else sizes[tested - 1])
        table = list(ab) if ab is not None else AB
        idx = (np.arange(m) - int(sel[0]) + seed) % len(table)
        self.a = np.array([table[i][0] for i in idx], np.float64)
        self.b = np.array([table[i][1] for i in idx], np.float64)
        shift = pole_shift if pole_shift is not None else (POLE_SHIFT if act == "reciprocal" else 0.0)
        self.b = self.b + shift
        self.tap = (5 * np.arange(m) + seed) % k
        self.layers: E.Layers = []
        kk = n_in
        for li, mm in enumerate(sizes):
            W, b = np.zeros((kk, mm)), np.zeros(mm)
            if li < tested:
                W[np.arange(mm) % kk, np.arange(mm)] = 1.0
            elif li == tested:
                W[self.tap, np.arange(mm)] = self.a
                b = self.b.copy()
            else:
                W[self.src[li], np.arange(mm)] = 1.0
            self.layers.append((W, b))
            kk = mm
        self.acts = ["identity"] * L
        self.acts[tested] = act
        if tested < L - 1:
            self.acts[L - 1] = post_act

    @property
    def classification(self) -> bool:
        return self.n_out > 1

    def pmml(self, normalization: Optional[str] = None, net_normalization: Optional[str] = None) -> str:
        thr = [None] * len(self.sizes)
        thr[self.tested] = self.layer_thr
        return E.nn_pmml(self.layers, self.classification, normalization, activations=self.acts, thresholds=thr,
                         net_threshold=self.net_thr, net_normalization=net_normalization)

    def z_all(self, X: np.ndarray) -> np.ndarray:
        """float64 ``[rows, units]`` pre-activations of the tested layer (NaN inputs as 0); asserts
        the exactness guard: multiples of 1/32 below 2^24, and a bf16-exact chain below the layer."""
        H = np.nan_to_num(np.asarray(X, np.float64))
        chain = [H]
        for li in range(self.tested):
            H = H @ self.layers[li][0]
            chain.append(H)
        Z = H @ self.layers[self.tested][0] + self.layers[self.tested][1]
        E.assert_exact([Z] + chain, dyadic=1.0 / 32)
        for v in chain + [self.a]:
            assert np.array_equal(bf16_rn(v.astype(F32)).astype(np.float64), v), "operand is not a bf16 number"
        return Z

    def reference(self, X: np.ndarray):
        """``(out [rows, n_out] float64, valid [rows], z [rows, n_out])``: ``activate`` in float64 on the
        exact z of the units the outputs read; ``valid`` is the input stage's (no NaN cell)."""
        Z = self.z_all(X)[:, self.sel]
        out = activate(self.act, Z, self.thr)
        if self.tested < len(self.sizes) - 1 and self.post_act != "identity":
            out = activate(self.post_act, out, 0.0)
        return out, ~np.isnan(np.asarray(X, np.float64)).any(axis=1), Z

    def unread_poles(self, X: np.ndarray) -> int:
        """Entries of the tested layer that are not finite in float64 or overflow fp32, on a unit no
        output reads (the dense kernels multiply them by a stored zero; the oracle never sees them)."""
        Z = self.z_all(X)
        with np.errstate(all="ignore"):
            A = np.abs(activate(self.act, Z, self.thr))
        bad = ~(A <= np.finfo(F32).max)
        bad[:, np.unique(self.sel)] = False
        return int(bad[~np.isnan(np.asarray(X, np.float64)).any(axis=1)].sum())


def ramp_matrix(rows: int, n_in: int, seed: int = 0, quarter: bool = False) -> np.ndarray:
    """fp32 ``[rows, n_in]`` of ``m / 16``, ``|m| <= 64``: column c is ``((r s_c + o_c) % 129 - 64) / 16``
    with s_c prime to 129, so any 129 consecutive rows hold every grid value in every column (the
    ends +-4 and 0 included) and rows r, r + 129 repeat each other. ``quarter``: multiples of 1/4
    instead (33 values). Every cell equal to zero with r + c odd is ``-0.0``; every 37th row from
    row 5 carries one NaN (their residues mod 129 differ, so no grid value is lost); row 0 is zero."""
    steps = [s for s in range(1, 129) if s % 3 and s % 43]
    r = np.arange(rows)[:, None]
    c = np.arange(n_in)[None, :]
    s = np.array([steps[(j + seed) % len(steps)] for j in range(n_in)])[None, :]
    if quarter:
        X = (((r * s + 16 + 5 * c) % 33) - 16) / 4.0
    else:
        X = (((r * s + 64 + 17 * c) % 129) - 64) / 16.0
    X[0] = 0.0
    X = X.astype(F32)
    X[(X == 0) & ((r + c) % 2 == 1)] = -0.0
    for rr in range(5, rows, 37):
        X[rr, (7 * rr) % n_in] = np.nan
    return X


# --------------------------------------------------------------------------- the device formulas (numpy twin)


def twin_activate(act: str, z, thr: float = 0.0) -> np.ndarray:
    """``nn_act.h::activate`` in fp32 numpy, the same operations in the same order."""
    z = np.asarray(z, F32)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        if act == "logistic":
            return one / (one + np.exp(-z))
        if act == "tanh":
            return np.tanh(z)
        if act == "rectifier":
            return np.maximum(z, F32(0.0))
        if act == "exponential":
            return np.exp(z)
        if act == "reciprocal":
            return one / z
        if act == "square":
            return z * z
        if act == "Gauss":
            return np.exp(-z * z)
        if act == "sine":
            return np.sin(z)
        if act == "cosine":
            return np.cos(z)
        if act == "Elliott":
            return z / (one + np.abs(z))
        if act == "arctan":
            return F32(0.63661977236758134) * np.arctan(z)
        if act == "threshold":
            return np.where(z > F32(thr), one, F32(0.0))
    assert act == "identity", act
    return z


def activation_mutants(act: str, layer_thr_set: bool) -> Dict[str, callable]:
    """Named wrong versions of the tested layer's activation: ``f(z32, thr) -> fp32``. Every one must
    leave the comparison rule of its case (a changed bit, or more than the bound)."""
    out = {f"code {other} for {act}": (lambda z, t, o=other: twin_activate(o, z, t)) for other in ACTS if other != act}
    one = F32(1.0)
    if act == "threshold":
        out[">= for >"] = lambda z, t: np.where(z >= F32(t), one, F32(0.0))
        if layer_thr_set:
            out["network threshold where the layer sets one"] = lambda z, t: twin_activate("threshold", z, NET_THR)
    if act == "arctan":
        out["arctan without 2/pi"] = lambda z, t: np.arctan(z)
    if act == "Gauss":
        out["Gauss with +z^2"] = lambda z, t: np.exp(z * z)
    if act == "logistic":
        out["logistic without the negation"] = lambda z, t: one / (one + np.exp(z))
    if act == "cosine":
        out["sine for cosine"] = lambda z, t: np.sin(z)
    if act == "reciprocal":
        # a padded unit (weights 0, bias 0) holds 1/0 = inf unless it is re-zeroed (mlp.hip::rfinish)
        # or padded with a finite bias: the next layer's stored zero times inf is NaN on every row.
        # The same slip after exponential / cosine leaves f(0) = 1 times a zero weight: no change,
        # so it is no mutant there.
        out["padded units keep reciprocal(0)"] = lambda z, t: twin_activate("reciprocal", z, t) + F32(0.0) * F32(np.inf)
    return out


def expected(ramp: Ramp, X: np.ndarray, bf16_hidden: bool):
    """``(want fp32 [rows, n_out], tol float64 or None, ref64, valid, z)``: ``tol`` None means bit for bit
    against ``want``; else ``|device - ref64| <= tol``. ``bf16_hidden``: a bf16 kernel carries the tested
    (hidden) layer's activation as bf16."""
    ref, valid, z = ramp.reference(X)
    with np.errstate(over="ignore"):
        want = ref.astype(F32)
    if bf16_hidden:
        want = bf16_rn(want)
    exact = ramp.act in EXACT_ACTS and ramp.post_act in EXACT_ACTS
    return want, (None if exact else bound(ramp.act, z, ref, bf16_hidden)), ref, valid, z


def caught(got: np.ndarray, want: np.ndarray, tol, ref: np.ndarray, valid: np.ndarray) -> bool:
    """Does the comparison rule reject ``got``?"""
    g = np.asarray(got, F32)[valid]
    if tol is None:
        return not np.array_equal(E.bits(g), E.bits(want[valid]))
    return bool((~(np.abs(g.astype(np.float64) - ref[valid]) <= tol[valid])).any())


# --------------------------------------------------------------------------- row normalisation

NORMS = ("softmax", "simplemax", None)


class Logits(Ramp):
    """Small-logit network: identity everywhere, the output layer under "test" with ``a_u`` from
    +-1..3 and small integer biases, inputs in multiples of 1/4: logits ``k / 4``, ``|k| <= 64``. The
    biases sum to zero (unit 0 balances them), so the all-zero row 0 has a logit sum of exactly 0;
    from four outputs on, the last unit copies unit ``dup`` (equal logits on every row)."""

    def __init__(self, n_in: int, hidden: Sequence[int], n_out: int):
        A = [1, -1, 2, -2, 3, -3]
        ab = [(A[u % 6], float((3 * u + 1) % 7 - 3)) for u in range(n_out)]
        super().__init__(n_in, hidden, n_out, len(hidden), "identity", seed=0, ab=ab)
        k = self.layers[-1][0].shape[0]
        self.a = np.array([p[0] for p in ab], np.float64)
        self.b = np.array([p[1] for p in ab], np.float64)
        if n_out >= 4:  # the copied unit: the one of 1 .. n_out - 2 that is the maximum on most rows
            H = np.nan_to_num(self.matrix(ROWS).astype(np.float64))
            for W, _ in self.layers[:-1]:
                H = H @ W
            Zp = H[:, self.tap] * self.a + self.b
            d = self.dup = 1 + int(np.bincount(Zp[:, 1:-1].argmax(axis=1), minlength=n_out - 2).argmax())
            self.a[-1], self.b[-1], self.tap[-1] = self.a[d], self.b[d], self.tap[d]
        # unit 0 balances: the biases sum to 0 and the weights to a power of two (or minus one), so
        # the rows of all +1 / all -1 inputs (``matrix``) have the logit sums +-sum(a): one is 2^j
        rest = self.a[1:].sum()
        self.a[0] = min((t - rest for t in (1, 2, 4, -1, -2, -4) if t != rest), key=abs)
        self.b[0] = -self.b[1:].sum()
        assert 1 <= abs(self.a[0]) <= 4
        W = np.zeros((k, n_out))
        W[self.tap, np.arange(n_out)] = self.a
        self.layers[-1] = (W, self.b.copy())

    def matrix(self, rows: int) -> np.ndarray:
        """``ramp_matrix`` in multiples of 1/4 with row 1 all +1 and row 2 all -1."""
        X = ramp_matrix(rows, self.n_in, quarter=True)
        X[1:2], X[2:3] = 1.0, -1.0
        return X

    def logits(self, X: np.ndarray):
        Z = self.z_all(X)
        E.assert_exact([Z, np.abs(Z).sum(axis=1)], dyadic=0.25)
        assert np.abs(Z).max() <= 16.0
        return Z, ~np.isnan(np.asarray(X, np.float64)).any(axis=1)


def norm_reference(Z: np.ndarray, norm: Optional[str]):
    """``(P float64, label (first maximum of P), S)``: ``normalize_layer`` in float64; S is the softmax
    bound's scale ``p (1 + mx - z_u) + (n_out - 1) p`` (the exponent's argument error and the n-term sum)."""
    with np.errstate(all="ignore"):
        P = normalize_layer(norm, Z)
    S = None
    if norm == "softmax":
        S = P * (1.0 + Z.max(axis=1, keepdims=True) - Z) + (Z.shape[1] - 1) * P
    return P, np.argmax(P, axis=1), S


def twin_normalize(Z, norm: Optional[str], mutant: Optional[str] = None, width: int = 32):
    """The four device copies (mlp.hip panel epilogue and repilogue, gemm.hip decode_row and the
    streaming decode) share one formula: fp32 ``mx``, ``e_u = exp(z_u - mx)`` (softmax) or ``z_u``,
    an in-order fp32 sum, ``p_u = e_u / sum``, first maximum of p. Returns ``(p fp32, label)``.
    Mutants: ``padded-sum`` (the 32-wide tile's padded units, logit 0, join the sum), ``half-sum``
    (the sum of one lane half: units with ``u % 8 < 4``), ``abs-sum`` (simplemax over |z|), ``last-tie``."""
    Z = np.asarray(Z, F32)
    n = Z.shape[1]
    with np.errstate(all="ignore"):
        mx = Z.max(axis=1, keepdims=True)
        Ev = np.exp(Z - mx) if norm == "softmax" else Z
        terms = np.abs(Ev) if mutant == "abs-sum" else Ev
        if mutant == "half-sum":
            terms = terms[:, (np.arange(n) % 8) < 4]
        s = np.zeros(len(Z), F32)
        for u in range(terms.shape[1]):
            s = s + terms[:, u]
        if mutant == "padded-sum" and n < width:
            pad = np.exp(-mx[:, 0]) if norm == "softmax" else np.zeros(len(Z), F32)
            for _ in range(width - n):
                s = s + pad
        P = Ev / s[:, None] if norm else Ev
    Pn = np.where(np.isnan(P), -np.inf, P)
    label = (n - 1 - np.argmax(Pn[:, ::-1], axis=1)) if mutant == "last-tie" else np.argmax(Pn, axis=1)
    return P, label


def norm_mutants(norm: Optional[str], n_out: int) -> List[str]:
    out = ["last-tie"] if n_out >= 4 else []
    half = ["half-sum"] if n_out > 4 else []  # units 0..3 all sit in one lane half
    if norm == "softmax":
        out += half + (["padded-sum"] if n_out < 32 else [])
    if norm == "simplemax":
        out += half + ["abs-sum"]
    return out


# --------------------------------------------------------------------------- kernel paths

# name -> (n_in, hidden, n_out, tested layers; the last index is the output site)
FUSED_PATHS = {
    "17-33-1": (17, (33,), 1, (0, 1)),
    "21-50-33-7": (21, (50, 33), 7, (0, 1, 2)),
    "64-256-256-1": (64, (256, 256), 1, (0, 1, 2)),  # bf16: the register kernel, output layer folded
    "64-256-256-7": (64, (256, 256), 7, (0, 1, 2)),  # bf16: the register kernel, staged output layer
    "16-32x7-1": (16, (32,) * 7, 1, (3,)),
}
WIDE_PATHS = {
    "33-300-1": (33, (300,), 1, (0, 1)),
    "65-257-300-1": (65, (257, 300), 1, (0, 1)),
    "8-300-33": (8, (300,), 33, (0, 1)),  # output groups + streaming decode
    "24-512-768-4": (24, (512, 768), 4, (0, 1, 2)),  # fused head (bf16) on and off
}
PATHS = {**FUSED_PATHS, **WIDE_PATHS}
SITES = [(name, t) for name, p in PATHS.items() for t in p[3]]
# the two-site cases: rectifier in the hidden layer, square in the output layer (both exact): the
# activations of the two sites swapped show on every row with z < 0
TWO_SITE = ("17-33-1", "33-300-1")
SEEDS = (0, 1)
ROWS = 257

# output widths of the normalisation probes: name -> (n_in, hidden, n_out)
NORM_FUSED = {"12-40-2": (12, (40,), 2), "12-40-7": (12, (40,), 7), "12-40-32": (12, (40,), 32),
              "64-256-256-4": (64, (256, 256), 4), "64-256-256-7": (64, (256, 256), 7)}
NORM_WIDE = {"24-512-768-4": (24, (512, 768), 4), "8-300-33": (8, (300,), 33), "8-300-40": (8, (300,), 40)}


def ramp(name: str, tested: int, variant, seed: int, **kw) -> Ramp:
    n_in, hidden, n_out, _ = PATHS[name]
    _, act, lthr, nthr = variant
    return Ramp(n_in, hidden, n_out, tested, act, seed, layer_thr=lthr, net_thr=nthr, **kw)


def is_output_site(name: str, tested: int) -> bool:
    return tested == len(PATHS[name][1])
