"""Exact probes for the derive kernel (csrc/derive.hip): the ``[rows, n_sel]`` fp32 matrix and ``row_ok``.

Two families of documents, each a ``RegressionModel`` behind a ``TransformationDictionary``:

* **exact** — ``+ - *``, division by powers of two, comparisons, rounding functions, the n-ary
  aggregates, ``if`` / ``and`` / ``or``, ``modulo``, ``NormContinuous`` (knots spaced by powers of two),
  ``NormDiscrete``, ``Discretize``, ``MapValues``, ``isIn`` and string copies. Inputs and constants lie on
  the grid ``k / 8`` (``|k| <= 64``) plus the fp32 specials, so every intermediate is an exact float64
  in any evaluation order, fused or not. :class:`Reference` evaluates the parsed expression trees
  (``pmml.ir``) one row at a time in Python floats and checks every arithmetic result against
  ``fractions.Fraction``; a row with an inexact intermediate is dropped by the builder (``FLT_MAX +
  1/8``) and the final table asserts that none is left. A stored value is rounded to fp32 once,
  to nearest even, which is what ``(float)v`` does; columns that another derived field reads hold
  exact fp32 values (asserted), except in the document that pins the fp32 column itself.
* **rounded** — general ``/``, ``sqrt``, ``pow``, ``hypot``, ``atan2``, the exponentials, logarithms,
  trigonometric and hyperbolic functions, ``erf`` and the normal distribution functions, one
  function per derived field, straight from the inputs. The reference is ``mpmath`` at 400 bits,
  rounded to float64 and then to fp32. Its fp32 bits are those of *any* float64 implementation
  whose relative error is below ``2^-40``, provided the true value is not within ``2^-40`` (relative)
  of an fp32 rounding midpoint; the builder replaces a probe input that violates this and
  ``test_derive_cases.py`` asserts that no probe of the final table does. Zero, infinite and NaN
  arguments take the values C99 Annex F fixes (sign of zero included).

Beside the reference: :func:`twin`, a restatement of ``runtime/derive.py::emulate`` with named mutants,
and :func:`launch_direct`, a ctypes call of ``pmml_derive_launch`` on a chosen input layout with
guard elements around both outputs."""

import functools
import math
import struct
from fractions import Fraction
from typing import Dict, List, Optional, Sequence

import numpy as np

from flink_jpmml_amd.pmml import ir

F32 = np.float32
NAN = float("nan")
INF = float("inf")
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = float(np.finfo(F32).tiny)
FLT_SUB = 2.0 ** -149
BIG_INT = 2.0 ** 24 + 2
NS = "http://www.dmg.org/PMML-4_4"
DTB = 128
ROW_COUNTS = (1, 127, 128, 129, 257)
SPECIALS = (0.0, -0.0, NAN, FLT_SUB, FLT_MIN, FLT_MAX, BIG_INT, INF, -INF)
MID_REL = 2.0 ** -40
GUARD = 64
SENTINEL32 = 0x5A5A5A5A


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32)


def same_bits(got, ref) -> np.ndarray:
    """Element-wise: equal fp32 bit patterns (the sign of zero counts), or NaN on both sides."""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    return (bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))


def f32(v: float) -> float:
    """float64 -> fp32, round to nearest even (overflow to inf, gradual underflow)."""
    if v != v or v in (INF, -INF):
        return v
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:
        return math.copysign(INF, v)


# --------------------------------------------------------------------------- document builders


def num(v) -> str:
    v = float(v)
    return str(int(v)) if v == int(v) and not (v == 0 and math.copysign(1, v) < 0) and abs(v) < 2 ** 31 else repr(v)


def _attrs(mm, dv) -> str:
    return (f' mapMissingTo="{mm}"' if mm is not None else "") + (f' defaultValue="{dv}"' if dv is not None else "")


def K(v) -> str:
    return f"<Constant>{v if isinstance(v, str) else num(v)}</Constant>"


def R(field: str, mm=None) -> str:
    return f'<FieldRef field="{field}"{_attrs(mm, None)}/>'


def A(fn: str, *args: str, mm=None, dv=None) -> str:
    return f'<Apply function="{fn}"{_attrs(mm, dv)}>{"".join(args)}</Apply>'


def NC(field: str, knots: Sequence, outliers: str = "asIs", mm=None) -> str:
    return (f'<NormContinuous field="{field}" outliers="{outliers}"{_attrs(mm, None)}>'
            + "".join(f'<LinearNorm orig="{num(o)}" norm="{num(n)}"/>' for o, n in knots) + "</NormContinuous>")


def ND(field: str, value: str, mm=None) -> str:
    return f'<NormDiscrete field="{field}" value="{value}"{_attrs(mm, None)}/>'


def DZ(field: str, bins: Sequence, mm=None, dv=None) -> str:
    """bins: (binValue, closure, left or None, right or None)."""
    out = f'<Discretize field="{field}"{_attrs(mm, dv)}>'
    for val, clo, lo, hi in bins:
        out += (f'<DiscretizeBin binValue="{val}"><Interval closure="{clo}"'
                + (f' leftMargin="{num(lo)}"' if lo is not None else "")
                + (f' rightMargin="{num(hi)}"' if hi is not None else "") + "/></DiscretizeBin>")
    return out + "</Discretize>"


def MV(fields: Sequence[str], rows: Sequence[Sequence], mm=None, dv=None) -> str:
    """rows: (key_0, .., key_{k-1}, out) literals."""
    out = f'<MapValues outputColumn="out"{_attrs(mm, dv)}>'
    out += "".join(f'<FieldColumnPair field="{f}" column="k{j}"/>' for j, f in enumerate(fields))
    out += "<InlineTable>"
    for row in rows:
        out += "<row>" + "".join(f"<k{j}>{v}</k{j}>" for j, v in enumerate(row[:-1])) + f"<out>{row[-1]}</out></row>"
    return out + "</InlineTable></MapValues>"


COLOURS = ("red", "green", "blue")


def document(inputs: Sequence[str], fields: Sequence[tuple], selected: Sequence[str],
             strings: Sequence[str] = (), data_attrs: Optional[Dict[str, str]] = None,
             mining_attrs: Optional[Dict[str, str]] = None) -> str:
    """``fields``: (name, dataType, body); ``strings``: the categorical string inputs (values COLOURS);
    ``selected``: the columns the regression reads, in order (coefficient 1 each)."""
    dd = ""
    for f in inputs:
        if f in strings:
            dd += (f'<DataField name="{f}" optype="categorical" dataType="string">'
                   + "".join(f'<Value value="{v}"/>' for v in COLOURS) + "</DataField>")
        else:
            dd += f'<DataField name="{f}" optype="continuous" dataType="double">{(data_attrs or {}).get(f, "")}</DataField>'
    dd += '<DataField name="y" optype="continuous" dataType="double"/>'
    td = ""
    for name, dtype, body in fields:
        optype = "categorical" if dtype == "string" else "continuous"
        td += f'<DerivedField name="{name}" optype="{optype}" dataType="{dtype}">{body}</DerivedField>\n'
    ms = '<MiningField name="y" usageType="target"/>' + "".join(
        f'<MiningField name="{f}"{(mining_attrs or {}).get(f, "")}/>' for f in inputs)
    preds = "".join(f'<NumericPredictor name="{s}" coefficient="1"/>' for s in selected)
    return (f'<PMML version="4.4" xmlns="{NS}"><DataDictionary>{dd}</DataDictionary>'
            f'<TransformationDictionary>\n{td}</TransformationDictionary>'
            f'<RegressionModel functionName="regression"><MiningSchema>{ms}</MiningSchema>'
            f'<RegressionTable intercept="0">{preds}</RegressionTable></RegressionModel></PMML>')


# --------------------------------------------------------------------------- rounded family (mpmath)

ROUNDED_UNARY = ("sqrt", "exp", "ln", "log10", "expm1", "ln1p", "sin", "cos", "tan", "asin", "acos", "atan", "sinh",
                 "cosh", "tanh", "erf", "stdNormalCDF", "stdNormalPDF", "stdNormalIDF")
ROUNDED_BINARY = ("/", "pow", "hypot", "atan2")


def _mp():
    import mpmath

    mpmath.mp.prec = 400
    return mpmath


def _c99(fn: str, a: float, b: float = 0.0) -> float:
    """Zero, infinite or NaN arguments, and arguments outside the domain: the values C99 Annex F
    fixes (Python's ``math`` returns them or raises; a domain error is NaN, a pole an infinity)."""
    if fn == "/":
        if b == 0.0:
            return NAN if (a == 0.0 or a != a) else math.copysign(INF, a) * math.copysign(1.0, b)
        return a / b
    if fn == "stdNormalCDF":
        return NAN if a != a else (0.0 if a == -INF else 1.0 if a == INF else 0.5)
    if fn == "stdNormalPDF":
        return NAN if a != a else 0.0  # +-inf only: a zero argument is an ordinary value
    if fn == "stdNormalIDF":
        return -INF if a == 0.0 else INF if a == 1.0 else NAN
    if fn in ("ln", "log10", "ln1p"):
        x = a + 1.0 if fn == "ln1p" else a
        if fn == "ln1p" and a == 0.0:
            return a  # keeps the sign of zero
        if x == 0.0:
            return -INF
        if x < 0.0 or x != x:
            return NAN
        return INF
    if fn == "pow" and a == 0.0 and b < 0.0:  # a pole: +inf, -inf for -0.0 under an odd integer exponent
        odd = math.isfinite(b) and b == int(b) and int(b) % 2 == 1
        return math.copysign(INF, a) if odd else INF
    f = {"sqrt": math.sqrt, "exp": math.exp, "expm1": math.expm1, "sin": math.sin, "cos": math.cos, "tan": math.tan,
         "asin": math.asin, "acos": math.acos, "atan": math.atan, "sinh": math.sinh, "cosh": math.cosh,
         "tanh": math.tanh, "erf": math.erf, "pow": math.pow, "hypot": math.hypot, "atan2": math.atan2}[fn]
    try:
        return f(a, b) if fn in ROUNDED_BINARY else f(a)
    except ValueError:
        return NAN
    except OverflowError:
        return INF


def _ordinary(v: float) -> bool:
    return v == v and v not in (INF, -INF) and v != 0.0


def rounded_value(fn: str, a: float, b: float = 0.0):
    """``(fp32 value as float, margin)`` of a rounded-family function. ``margin``: the distance of the
    true value from the nearer fp32 rounding midpoint, relative to the value (``inf`` where the value
    is fixed by C99 or exact)."""
    return _rounded_value(fn, struct.pack("dd", a, b))  # keyed on the bits: -0.0 is not +0.0


@functools.lru_cache(maxsize=None)
def _rounded_value(fn: str, key: bytes):
    a, b = struct.unpack("dd", key)
    binary = fn in ROUNDED_BINARY
    if not _ordinary(a) and not (fn == "stdNormalPDF" and a == 0.0) or (binary and not _ordinary(b)):
        return f32(_c99(fn, a, b)), INF
    if (fn in ("ln", "log10", "sqrt") and a < 0) or (fn == "ln1p" and a <= -1) or (fn in ("asin", "acos") and abs(a) > 1) \
            or (fn == "pow" and a < 0 and b != int(b)) or (fn == "stdNormalIDF" and not 0 < a < 1):
        return f32(_c99(fn, a, b)), INF
    mp = _mp()
    x, y = mp.mpf(a), mp.mpf(b)
    t = {"/": lambda: x / y, "pow": lambda: mp.power(x, y), "hypot": lambda: mp.sqrt(x * x + y * y),
         "atan2": lambda: mp.atan2(x, y), "sqrt": lambda: mp.sqrt(x), "exp": lambda: mp.exp(x), "ln": lambda: mp.log(x),
         "log10": lambda: mp.log10(x), "expm1": lambda: mp.expm1(x), "ln1p": lambda: mp.log1p(x),
         "sin": lambda: mp.sin(x), "cos": lambda: mp.cos(x), "tan": lambda: mp.tan(x), "asin": lambda: mp.asin(x),
         "acos": lambda: mp.acos(x), "atan": lambda: mp.atan(x), "sinh": lambda: mp.sinh(x), "cosh": lambda: mp.cosh(x),
         "tanh": lambda: mp.tanh(x), "erf": lambda: mp.erf(x), "stdNormalCDF": lambda: mp.ncdf(x),
         "stdNormalPDF": lambda: mp.npdf(x), "stdNormalIDF": lambda: mp.sqrt(2) * mp.erfinv(2 * x - 1)}[fn]()
    if t == 0:
        return 0.0, INF
    sign = -1.0 if t < 0 else 1.0
    m = abs(t)
    if m >= mp.mpf(2) ** 129:
        return sign * INF, INF
    if m < mp.mpf(2) ** -160:
        return sign * 0.0, INF
    y32 = abs(f32(float(m)))  # float(): nearest float64; then nearest fp32. Checked against the midpoints below
    top = mp.mpf(2) ** 128
    cur = top if y32 == INF else mp.mpf(y32)  # 2^128 stands for the infinity: FLT_MAX's upper midpoint is halfway to it
    below = mp.mpf(FLT_MAX) if y32 == INF else mp.mpf(float(np.nextafter(F32(y32), F32(-INF))))
    above = top if y32 >= FLT_MAX else mp.mpf(float(np.nextafter(F32(y32), F32(INF))))
    lo_mid, hi_mid = (below + cur) / 2, (cur + above) / 2
    margin = INF if m == cur else float(min(abs(m - lo_mid), abs(m - hi_mid)) / m)
    if y32 != INF:
        assert lo_mid <= m <= hi_mid, (fn, a, b)
    else:
        assert m >= lo_mid, (fn, a, b)
        margin = float(abs(m - lo_mid) / m)
    return sign * y32, margin


# --------------------------------------------------------------------------- the reference


class Reference:
    """Row-at-a-time evaluation of a compiled document's ``DerivedField`` trees in plain Python.
    ``fp32_columns``: a derived field is read back by later ones as the fp32 value the tile holds
    (the device's rule); ``False`` keeps float64 (the oracle's). After :meth:`columns`:
    ``inexact`` (rows with an inexact float64 intermediate), ``rounded_store`` (name -> rows whose
    stored value was rounded) and ``margins`` (every midpoint margin of the rounded family)."""

    def __init__(self, c, fp32_columns: bool = True):
        self.schema = c.schema
        self.defs = list(c.doc.transformations)
        self.inputs = list(c.active_fields)
        self.fp32_columns = fp32_columns
        self.read = set()
        for d in self.defs:
            self._reads(d.expression)

    def _reads(self, ex) -> None:
        if isinstance(ex, (ir.FieldRef, ir.NormContinuous, ir.NormDiscrete, ir.Discretize)):
            self.read.add(ex.field)
        elif isinstance(ex, ir.MapValues):
            self.read.update(f for f, _ in ex.field_columns)
        elif isinstance(ex, ir.Apply):
            for a in ex.args:
                self._reads(a)

    # -- exactness guard
    def _check(self, r: float, exact: Fraction) -> float:
        if not (math.isfinite(r) and Fraction(r) == exact):
            self._bad = True
        return r

    def _arith(self, fn: str, a: float, b: float) -> float:
        fin = math.isfinite(a) and math.isfinite(b)
        if fn == "+":
            return self._check(a + b, Fraction(a) + Fraction(b)) if fin else a + b
        if fn == "-":
            return self._check(a - b, Fraction(a) - Fraction(b)) if fin else a - b
        if fn == "*":
            return self._check(a * b, Fraction(a) * Fraction(b)) if fin else a * b
        if b == 0.0 or not fin:
            return _c99("/", a, b)
        return self._check(a / b, Fraction(a) / Fraction(b))

    def _sum(self, vals: Sequence[float]) -> float:
        acc = 0.0
        for v in vals:
            acc = self._arith("+", acc, v)
        return acc

    @staticmethod
    def _modulo(a: float, b: float) -> float:
        """The remainder takes the divisor's sign, a zero remainder too (numpy.mod); fmod is exact."""
        if a != a or b != b or a in (INF, -INF) or b == 0.0:
            return NAN
        r = a if b in (INF, -INF) else math.fmod(a, b)
        if r == 0.0:
            return math.copysign(0.0, b)
        if (r < 0.0) != (b < 0.0):
            r += b  # exact on the grid; +-inf for an infinite divisor of the other sign
        return r

    @staticmethod
    def _min(vals: Sequence[float], sign: float) -> float:
        """Java's Math.min / Math.max: -0.0 orders below +0.0 (``sign`` -1: max)."""
        best = vals[0]
        for v in vals[1:]:
            if sign * v < sign * best or (v == best == 0.0 and sign * math.copysign(1.0, v) < sign * math.copysign(1.0, best)):
                best = v
        return best

    def _lookup(self, field: str, lit) -> float:
        return self.schema.lookup(field, lit)

    # -- expressions
    def _apply(self, ex: ir.Apply, env) -> float:
        fn = ex.function
        mm = NAN if ex.map_missing_to is None else float(ex.map_missing_to)
        dv = NAN if ex.default_value is None else float(ex.default_value)
        if fn in ("isIn", "isNotIn"):
            v = env[ex.args[0].field]
            if v != v:
                return mm
            field = ex.args[0].field
            hit = any(v == self._lookup(field, a.value) for a in ex.args[1:])
            return float(hit == (fn == "isIn"))
        if fn == "if":  # neither attribute applies to ``if`` and ``isMissing``. Only the taken branch is
            cond = self._ev(ex.args[0], env, None)  # evaluated: the kernel computes both and selects, and
            pick = 1 if cond == 1.0 else 2 if cond == 0.0 else 0  # what it discards need not be exact
            return self._ev(ex.args[pick], env, None) if 0 < pick < len(ex.args) else NAN
        args = [self._ev(a, env, None) for a in ex.args]
        if fn in ("isMissing", "isNotMissing"):
            return float((args[0] != args[0]) == (fn == "isMissing"))
        present = [v for v in args if v == v]
        if fn in ("min", "max", "sum", "avg", "product", "median"):
            if not present:
                return mm
            if fn == "min":
                r = self._min(present, 1.0)
            elif fn == "max":
                r = self._min(present, -1.0)
            elif fn == "sum":
                r = self._sum(present)
            elif fn == "avg":
                r = self._arith("/", self._sum(present), float(len(present)))
            elif fn == "product":
                r = 1.0
                for v in present:
                    r = self._arith("*", r, v)
            else:
                s = sorted(present)  # stable: -0.0 and +0.0 compare equal and keep their argument order
                m = len(s)
                r = s[m // 2] if m & 1 else self._arith("*", 0.5, self._arith("+", s[m // 2 - 1], s[m // 2]))
        else:
            if len(present) != len(args):
                return mm
            a = args[0]
            b = args[1] if len(args) > 1 else 0.0
            if fn in ("+", "-", "*"):
                r = self._arith(fn, a, b)
            elif fn == "/" and not self.rounded:  # exact documents, and the fp32-column document (one IEEE division)
                r = self._arith("/", a, b)
            elif fn in ROUNDED_UNARY or fn in ROUNDED_BINARY:
                r, margin = rounded_value(fn, a, b)
                self._margins.append(margin)
            elif fn == "modulo":
                r = self._modulo(a, b)
            elif fn in ("and", "or"):
                t = [v != 0.0 for v in args]
                r = float(all(t) if fn == "and" else any(t))
            elif fn == "not":
                r = float(a == 0.0)
            elif fn == "abs":
                r = abs(a)
            elif fn == "floor":
                r = a if not math.isfinite(a) else math.copysign(float(math.floor(a)), a) if math.floor(a) == 0 else float(math.floor(a))
            elif fn == "ceil":
                r = a if not math.isfinite(a) else math.copysign(0.0, a) if math.ceil(a) == 0 else float(math.ceil(a))
            elif fn == "round":  # half up: floor(a + 0.5)
                s = a + 0.5  # one IEEE addition, nothing to reorder or fuse: exempt from the guard (2^-149 + 0.5)
                r = s if not math.isfinite(s) else math.copysign(0.0, s) if math.floor(s) == 0 else float(math.floor(s))
            elif fn == "rint":  # half to even
                r = a if not math.isfinite(a) else math.copysign(float(round(a)), a)
            else:
                cmp = {"equal": a == b, "notEqual": a != b, "lessThan": a < b, "lessOrEqual": a <= b,
                       "greaterThan": a > b, "greaterOrEqual": a >= b, "threshold": a > b}
                r = float(cmp[fn])
        if r != r and dv == dv:
            return dv
        return r

    def _ev(self, ex, env, out: Optional[str]) -> float:
        s = self.schema
        if isinstance(ex, ir.Constant):
            if ex.missing or ex.value is None:
                return NAN
            if out is not None and s.is_string(out):
                return float(s.code(out, ex.value))
            return float(ex.value)
        if isinstance(ex, ir.FieldRef):
            v = env[ex.field]
            if v != v and ex.map_missing_to is not None:
                v = self._lookup(out or ex.field, ex.map_missing_to)
            if out is not None and s.is_string(out) and s.is_string(ex.field) and out != ex.field:
                src = s.values.get(ex.field, [])
                v = float(s.code(out, src[int(v)])) if v == v and 0 <= v < len(src) else NAN
            return v
        if isinstance(ex, ir.NormContinuous):
            v = env[ex.field]
            if v != v:
                return NAN if ex.map_missing_to is None else float(ex.map_missing_to)
            o = [ln.orig for ln in ex.norms]
            n = [ln.norm for ln in ex.norms]
            if v < o[0] or v > o[-1]:
                if ex.outliers == "asMissingValues":
                    return NAN
                if ex.outliers == "asExtremeValues":
                    return n[0] if v < o[0] else n[-1]
            k = max(j for j in range(len(o) - 1) if j == 0 or o[j] <= v)
            if not math.isfinite(v):
                return n[k] + (v - o[k]) * (n[k + 1] - n[k]) / (o[k + 1] - o[k])
            exact = Fraction(n[k]) + (Fraction(v) - Fraction(o[k])) * (Fraction(n[k + 1]) - Fraction(n[k])) \
                / (Fraction(o[k + 1]) - Fraction(o[k]))
            for part in (Fraction(v) - Fraction(o[k]), (Fraction(v) - Fraction(o[k])) * (Fraction(n[k + 1]) - Fraction(n[k]))):
                self._check(float(part), part)
            r = float(exact)
            if r == 0.0:  # the sign of an exact zero sum: +0 unless both terms are -0
                r = n[k] + (v - o[k]) * (n[k + 1] - n[k]) / (o[k + 1] - o[k])
            return self._check(r, exact)
        if isinstance(ex, ir.NormDiscrete):
            v = env[ex.field]
            if v != v:
                return NAN if ex.map_missing_to is None else float(ex.map_missing_to)
            return float(v == self._lookup(ex.field, ex.value))
        if isinstance(ex, ir.Discretize):
            v = env[ex.field]
            tgt = out or "__bin__"
            if v != v:
                return NAN if ex.map_missing_to is None else self._lookup(tgt, ex.map_missing_to)
            for b in ex.bins:
                if b.interval.contains(v):
                    return self._lookup(tgt, b.bin_value)
            return NAN if ex.default_value is None else self._lookup(tgt, ex.default_value)
        if isinstance(ex, ir.MapValues):
            tgt = out or "__map__"
            keys = [env[f] for f, _ in ex.field_columns]
            if any(k != k for k in keys):
                return NAN if ex.map_missing_to is None else self._lookup(tgt, ex.map_missing_to)
            for row in ex.rows:
                if all(k == self._lookup(f, row.get(col)) for k, (f, col) in zip(keys, ex.field_columns)):
                    return self._lookup(tgt, row.get(ex.output_column))
            return NAN if ex.default_value is None else self._lookup(tgt, ex.default_value)
        assert isinstance(ex, ir.Apply), type(ex)
        return self._apply(ex, env)

    def columns(self, P: np.ndarray, names: Sequence[str], rounded: bool = False) -> np.ndarray:
        """fp32 ``[rows, len(names)]`` from the prepared matrix ``P``."""
        self.rounded = rounded
        n = len(P)
        out = np.empty((n, len(names)), F32)
        self.inexact = np.zeros(n, bool)
        self.rounded_store: Dict[str, List[int]] = {d.name: [] for d in self.defs}
        self.inexact_read: List[tuple] = []
        self._margins: List[float] = []
        col = {nm: j for j, nm in enumerate(names)}
        for r in range(n):
            env = {f: float(P[r, j]) for j, f in enumerate(self.inputs)}
            self._bad = False
            for d in self.defs:
                v = self._ev(d.expression, env, d.name)
                if d.data_type == "integer" and v == v and math.isfinite(v):
                    v = float(math.trunc(v)) if math.trunc(v) != 0 else math.copysign(0.0, v)
                s = f32(v)
                if s != v and v == v:
                    self.rounded_store[d.name].append(r)
                    if d.name in self.read:
                        self.inexact_read.append((d.name, r))
                env[d.name] = s if self.fp32_columns or d.data_type == "float" else v
                if d.name in col:
                    out[r, col[d.name]] = s
            for f in self.inputs:
                if f in col:
                    out[r, col[f]] = P[r, self.inputs.index(f)]
            self.inexact[r] = self._bad
        self.margins = np.array(self._margins)
        return out


# --------------------------------------------------------------------------- restated twin with mutants

MUTANTS = ("round-as-rint", "modulo-no-sign-rule", "modulo-no-signed-zero", "median-lower-middle",
           "minmax-propagate-nan", "minmax-numpy-zero-order", "if-any-nonzero-true", "default-before-mapmissing",
           "normcont-gt-for-ge", "normcont-extreme-returns-orig", "discretize-last-match-wins", "closure-bit0-flipped",
           "closure-bit1-flipped", "mapvalues-first-key-only", "integer-store-floor", "store-without-fp32-rounding",
           "row-ok-ignored")
# "normcont-gt-for-ge" cannot show on exact probes. It only moves an input that sits on an inner knot
# orig[k] from segment k to segment k - 1, and LinearNorms are continuous there: segment k - 1 gives
# nrm[k-1] + (orig[k] - orig[k-1]) * (nrm[k] - nrm[k-1]) / (orig[k] - orig[k-1]), which is nrm[k] when
# the arithmetic is exact, the value segment k gives too. test_derive_cases.py demonstrates it.
INERT_MUTANTS = ("normcont-gt-for-ge",)


def _java_minmax(st: np.ndarray, is_min: bool) -> np.ndarray:
    r = (np.nanmin if is_min else np.nanmax)(st, axis=0)
    zero = (st == 0) & (np.signbit(st) if is_min else ~np.signbit(st))
    return np.where((r == 0) & zero.any(axis=0), -0.0 if is_min else 0.0, r)


def _twin_apply(fn: int, args: List[np.ndarray], x: float, y: float, n: int, mutant: str) -> np.ndarray:
    from flink_jpmml_amd.runtime import derive as D

    if fn in (60, 61):
        m = np.isnan(args[0])
        return (m if fn == 60 else ~m).astype(np.float64)
    if fn == 62:
        cond = args[0]
        r = np.full(n, NAN)
        if len(args) > 1:
            true = (cond != 0.0) & ~np.isnan(cond) if mutant == "if-any-nonzero-true" else cond == 1.0
            r = np.where(true, args[1], r)
        if len(args) > 2:
            r = np.where(cond == 0.0, args[2], r)
        return r
    st = np.vstack(args)
    if 50 <= fn <= 55:
        miss = np.all(np.isnan(st), axis=0)
        st0 = np.where(miss[None, :], 0.0, st)
        if fn in (50, 51):
            if mutant == "minmax-propagate-nan":
                r = (np.min if fn == 50 else np.max)(st0, axis=0)
            elif mutant == "minmax-numpy-zero-order":
                r = (np.nanmin if fn == 50 else np.nanmax)(st0, axis=0)
            else:
                r = _java_minmax(st0, fn == 50)
        elif fn == 55:
            s = np.sort(st0, axis=0, kind="stable")  # NaN last; equal zeros keep their argument order
            m = (~np.isnan(st0)).sum(axis=0)
            cols = np.arange(n)
            lo, hi = s[np.maximum(m - 1, 0) // 2, cols], s[m // 2, cols]
            r = lo if mutant == "median-lower-middle" else np.where(m & 1, hi, 0.5 * (lo + hi))
        else:
            r = D._NP_NARY[fn](st0, axis=0)
    else:
        miss = np.any(np.isnan(st), axis=0)
        if fn in (56, 57):
            t = st != 0
            r = (np.all(t, axis=0) if fn == 56 else np.any(t, axis=0)).astype(np.float64)
        elif fn == 27 and mutant == "round-as-rint":
            r = np.rint(args[0])
        elif fn == 5 and mutant == "modulo-no-sign-rule":
            r = np.fmod(args[0], args[1])
            r = np.where(r == 0, np.copysign(0.0, args[1]), r)
        elif fn == 5 and mutant == "modulo-no-signed-zero":
            r = np.mod(args[0], args[1])
            r = np.where(r == 0, np.copysign(0.0, args[0]), r)
        elif fn in D._NP_UNARY:
            r = D._NP_UNARY[fn](args[0])
        else:
            r = D._NP_BINARY[fn](args[0], args[1]).astype(np.float64)
    r = np.asarray(r, dtype=np.float64)
    if mutant == "default-before-mapmissing":
        r = np.where(np.isnan(r) & ~np.isnan(y), y, r)
        return np.where(miss & np.isnan(r), x, r)
    r = np.where(miss, x, r)
    return np.where(~miss & np.isnan(r) & ~np.isnan(y), y, r)


def twin(prog, P: np.ndarray, ok: np.ndarray, mutant: str = ""):
    """``runtime/derive.py::emulate`` restated: ``(fp32 [rows, n_sel], row_ok uint8)`` of a prepared
    matrix and the preparation's row validity."""
    n = P.shape[0]
    wide = mutant == "store-without-fp32-rounding"
    tile = np.full((n, prog.n_tile), NAN, dtype=np.float64 if wide else F32)
    tile[:, : len(prog.inputs)] = np.asarray(P, dtype=F32)
    pool = prog.pool
    stack: List[np.ndarray] = []
    with np.errstate(all="ignore"):
        for op, a, b, c, x, y in prog.insns.tolist():
            if op == 0:
                stack.append(tile[:, a].astype(np.float64))
            elif op == 1:
                stack.append(np.full(n, x))
            elif op == 2:
                stack[-1] = np.where(np.isnan(stack[-1]), x, stack[-1])
            elif op == 3:
                v = stack[-1]
                okv = ~np.isnan(v) & (v >= 0) & (v < b)
                tab = np.append(pool[a: a + b], NAN)
                stack[-1] = np.where(okv, tab[np.where(okv, v, b).astype(np.int64)], NAN)
            elif op == 4:
                v = stack[-1]
                orig, nrm = pool[a: a + b], pool[a + b: a + 2 * b]
                seg = np.zeros(n, dtype=np.int64)
                for k in range(1, b - 1):
                    seg += (v > orig[k]) if mutant == "normcont-gt-for-ge" else (v >= orig[k])
                r = nrm[seg] + (v - orig[seg]) * (nrm[seg + 1] - nrm[seg]) / (orig[seg + 1] - orig[seg])
                lo, hi = v < orig[0], v > orig[-1]
                ends = (orig[0], orig[-1]) if mutant == "normcont-extreme-returns-orig" else (nrm[0], nrm[-1])
                if c == 1:
                    r = np.where(lo | hi, NAN, r)
                elif c == 2:
                    r = np.where(lo, ends[0], np.where(hi, ends[1], r))
                stack[-1] = np.where(np.isnan(v), x, r)
            elif op == 5:
                v = stack[-1]
                stack[-1] = np.where(np.isnan(v), y, (v == x).astype(np.float64))
            elif op == 6:
                v = stack[-1]
                r = np.full(n, y)
                done = np.isnan(v)
                for k in range(b):
                    lo_, hi_, clo, val = pool[a + 4 * k: a + 4 * k + 4]
                    clo = int(clo) ^ (1 if mutant == "closure-bit0-flipped" else 2 if mutant == "closure-bit1-flipped" else 0)
                    m = ((v > lo_) if clo & 1 else (v >= lo_)) & ((v < hi_) if clo & 2 else (v <= hi_)) & ~np.isnan(v)
                    if mutant != "discretize-last-match-wins":
                        m &= ~done
                    r = np.where(m, val, r)
                    done |= m
                stack[-1] = np.where(np.isnan(v), x, r)
            elif op == 7:
                keys = stack[len(stack) - c:] if c else []
                del stack[len(stack) - c:]
                anymiss = np.zeros(n, dtype=bool)
                for kv in keys:
                    anymiss |= np.isnan(kv)
                r = np.full(n, y)
                matched = np.zeros(n, dtype=bool)
                for i in range(b):
                    row = pool[a + i * (c + 1): a + (i + 1) * (c + 1)]
                    m = ~matched & ~anymiss
                    for j, kv in enumerate(keys[:1] if mutant == "mapvalues-first-key-only" else keys):
                        m &= kv == row[j]
                    r = np.where(m, row[c], r)
                    matched |= m
                stack.append(np.where(anymiss, x, r))
            elif op == 8:
                args = stack[len(stack) - b:]
                del stack[len(stack) - b:]
                stack.append(_twin_apply(a, args, x, y, n, mutant))
            elif op == 9:
                v = stack.pop()
                if c == 2:
                    v = np.where(np.isnan(v), v, np.floor(v) if mutant == "integer-store-floor" else np.trunc(v))
                tile[:, a] = v if wide else v.astype(F32)
        cols = tile[:, prog.out_cols].astype(F32)
    row_ok = np.ones(n, np.uint8) if mutant == "row-ok-ignored" else np.asarray(ok, bool).astype(np.uint8)
    return cols, row_ok


# --------------------------------------------------------------------------- input tables

GRID = np.arange(-64, 65) / 8.0


def _grid_rows(n: int, width: int, seed: int, nan_rate: float = 0.06) -> np.ndarray:
    rng = np.random.default_rng(seed)
    X = rng.integers(-64, 65, size=(n, width)) / 8.0
    X[rng.random(X.shape) < nan_rate] = NAN
    X[::7] = np.round(X[::7])  # integers: ties for comparisons, modulo and rounding
    return X


def apply_table() -> np.ndarray:
    """[rows, 6]: a, b, e, f, g continuous and the colour code c. Blocks placed by construction, then
    grid rows; ``build`` drops the rows its document cannot hold exactly."""
    rows: List[List[float]] = []
    g = [1.5, -2.25, 0.375, 4.0, -0.125]

    def row(a=g[0], b=g[1], e=g[2], f=g[3], gg=g[4], c=0.0):
        rows.append([a, b, e, f, gg, c])

    for i, sa in enumerate(SPECIALS):  # every pair of specials in (a, b); the other fields are zero, which
        for j, sb in enumerate(SPECIALS):  # keeps FLT_MAX + e + f + g exact
            row(a=sa, b=sb, e=0.0, f=0.0, gg=0.0, c=float((i + j) % 3))
    for s in SPECIALS:  # every special in e, f, g
        row(a=0.0, b=0.0, e=s, f=0.0, gg=0.0)
        row(a=0.0, b=0.0, e=0.0, f=s, gg=0.0)
        row(a=0.0, b=0.0, e=0.0, f=0.0, gg=s)
        row(a=s, b=1.0, e=0.0, f=0.0, gg=0.0)
        row(a=1.0, b=s, e=0.0, f=0.0, gg=0.0)
    for cc in (NAN, 0.0, -0.0, 1.0, 2.0):
        row(c=cc)
        row(a=NAN, c=cc)
    for k in range(-4, 5):  # k + 0.5: round half up against half even; the integer store
        row(a=k + 0.5, b=-(k + 0.5))
        row(a=float(k), b=k + 0.25)
    for a, b in ((5.5, 2.0), (-5.5, 2.0), (5.5, -2.0), (-5.5, -2.0), (4.0, 2.0), (4.0, -2.0), (-4.0, 2.0), (-4.0, -2.0),
                 (1.0, 0.0), (1.0, -0.0), (INF, 2.0), (-INF, 2.0), (1.0, INF), (-1.0, INF), (1.0, -INF), (-1.0, -INF),
                 (0.0, -3.0), (-0.0, 3.0), (0.0, 3.0), (7.875, 0.125), (-7.875, 8.0)):
        row(a=a, b=b)
    for cond in (1.0, 0.0, 2.0, -0.0, NAN, -1.0, 0.5):  # if: every condition x present / missing branches
        for then in (3.5, NAN):
            for other in (-2.25, NAN):
                row(a=cond, b=then, e=other)
    for a in (1.0, 0.0, NAN, 2.0, -0.0):  # and / or
        for b in (1.0, 0.0, NAN):
            row(a=a, b=b)
    five = ([5.0, 4.0, 3.0, 2.0, 1.0], [2.0, 2.0, 1.0, 2.0, 1.0], [1.0, 2.0, 3.0, 4.0, 5.0], [-1.5, -1.5, -1.5, -1.5, -1.5],
            [0.5, -0.0, 0.0, -0.5, 0.0], [8.0, -8.0, 7.875, -7.875, 0.125])
    for vals in five:  # the aggregates: descending order, duplicates, 0..5 arguments missing
        for mask in (0b00000, 0b00001, 0b10000, 0b00110, 0b01001, 0b11100, 0b00111, 0b11110, 0b01111, 0b11011, 0b11111):
            row(*[NAN if mask >> j & 1 else v for j, v in enumerate(vals)])
    for a, b in ((-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 0.0)):  # signed zeros of min / max, one and two missing
        row(a=a, b=b, e=NAN)
        row(a=a, b=b, e=1.0)
        row(a=a, b=b, e=-1.0)
    X = np.array(rows)
    fill = _grid_rows(1025 - len(X), 6, seed=11)
    fill[:, 5] = np.random.default_rng(12).choice([0.0, 1.0, 2.0, NAN], size=len(fill), p=[0.3, 0.3, 0.3, 0.1])
    return np.concatenate([X, fill])


def norm_table() -> np.ndarray:
    """[rows, 4]: a (every knot and bin edge with one fp32 ulp either side, the specials), b, and the
    colour codes c, c2."""
    edges = (-6.0, -4.0, -3.0, -2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 8.0)
    vals: List[float] = []
    for e in edges:
        e32 = F32(e)
        vals += [e, float(np.nextafter(e32, F32(-INF))), float(np.nextafter(e32, F32(INF)))]
    vals += list(SPECIALS) + [-FLT_MAX, -BIG_INT, -FLT_MIN, -FLT_SUB, -6.0, 6.0, 1.5, -1.5, 0.25, 2.5, 10.0, -10.0]
    rows = []
    for i, v in enumerate(vals):
        for j, b in enumerate((1.0, 2.0, NAN)):
            rows.append([v, b, float((i + j) % 3), float((i // 3 + j) % 3)])
    for c in (0.0, 1.0, 2.0, NAN, -0.0):
        for c2 in (0.0, 1.0, 2.0, NAN):
            for b in (1.0, 2.0, 3.0, NAN):
                rows.append([1.0, b, c, c2])
    X = np.array(rows)
    fill = _grid_rows(600 - len(X), 4, seed=21)
    rng = np.random.default_rng(22)
    fill[:, 1] = rng.choice([1.0, 2.0, 3.0, NAN], size=len(fill))
    fill[:, 2:] = rng.choice([0.0, 1.0, 2.0, NAN], size=(len(fill), 2), p=[0.3, 0.3, 0.3, 0.1])
    return np.concatenate([X, fill])


ROUNDED_A = (-13.0, -10.0, -8.5, -8.0, -6.0, -4.0, -1.0, 0.0, 8.5, 4.0, 100.0, 2.0, 3.0, 1.0, 0.5, 0.125, 0.25, 0.75, 0.875,
             2.0 ** -10, 1.0 - 2.0 ** -10, 2.0 ** -20, -0.5, 1.5, 2.5, 7.375, -3.625, 20.0, 88.0, 89.0, -100.0, -104.0, 700.0,
             10.0, 1000.0, 0.1015625, -0.9375, 5.625, -2.875, BIG_INT, FLT_MAX, FLT_MIN, FLT_SUB, -FLT_SUB, INF, -INF, NAN, -0.0,
             -2.0, 16.0, 1.0 / 3.0, 0.7, -0.3, 6.25)
ROUNDED_B = (3.0, 4.0, 2.0, 0.5, -1.0, 7.0, 0.0, -0.0, -2.5, 3.0, INF, NAN, -INF, 10.0, 1.0 / 3.0)


def rounded_table() -> np.ndarray:
    rows = [[float(F32(a)), float(F32(ROUNDED_B[(i + s) % len(ROUNDED_B)]))] for s in range(5) for i, a in enumerate(ROUNDED_A)]
    rows += [[2.0, 3.0], [3.0, 4.0], [4.0, 2.0], [100.0, 10.0], [0.0, 0.0], [-8.0, 1.0 / 3.0], [-8.0, 3.0], [-0.0, -1.0],
             [0.0, -1.0], [-0.0, 3.0], [-0.0, 2.0]]
    return np.array(rows, F32).astype(np.float64)


# --------------------------------------------------------------------------- the documents

KNOTS2 = ((-1.0, 0.0), (1.0, 1.0))
# no knot at 0: one fp32 ulp beside it is 2^-149, and 2^-149 - orig is not a float64
KNOTS3 = ((-3.0, -1.0), (-1.0, 0.5), (1.0, 4.0))
KNOTS5 = ((-6.0, 8.0), (-2.0, 6.0), (-1.0, 5.5), (1.0, 1.5), (5.0, -2.0))  # a decreasing norm


def apply_fields() -> List[tuple]:
    a, b, e, f, g = (R(x) for x in "abefg")
    F: List[tuple] = []

    def add(name, body, dtype="double"):
        F.append((name, dtype, body))

    for nm, fn in (("add", "+"), ("sub", "-"), ("mul", "*")):
        add(nm, A(fn, a, b))
    add("div8", A("/", a, K(8)))
    add("divhalf", A("/", b, K(-0.5)))
    for fn in ("equal", "notEqual", "lessThan", "lessOrEqual", "greaterThan", "greaterOrEqual", "threshold"):
        add("c_" + fn, A(fn, a, b))
    add("eq_arith", A("equal", A("+", A("*", a, K(0.5)), A("*", a, K(0.5))), A("/", A("*", a, K(4)), K(4))))
    for fn in ("abs", "floor", "ceil", "round", "rint", "not"):
        add("u_" + fn, A(fn, a))
        add("ub_" + fn, A(fn, b))
    add("mod", A("modulo", a, b))
    def show_zero(x):  # 1 / x where x is a zero: its sign shows as +-inf; any other value as it is
        return A("if", A("equal", x, K(0)), A("/", K(1), x), x)

    add("mod_inv", show_zero(A("modulo", a, b)))
    add("mod_dv", A("modulo", a, b, mm=-7, dv=9))
    for fn in ("min", "max"):
        add(fn + "2", A(fn, a, b))
        add(fn + "2_inv", show_zero(A(fn, a, b)))
        add(fn + "2r_inv", show_zero(A(fn, b, a)))
        add(fn + "3_inv", show_zero(A(fn, a, b, e)))
        add(fn + "5", A(fn, a, b, e, f, g, mm=-3))
    add("sum5", A("sum", a, b, e, f, g))
    add("sum1", A("sum", a, mm=2.5))
    add("avg1", A("avg", a))
    add("avg2", A("avg", a, b))
    add("avg4", A("avg", a, b, b, a, mm=0.25))
    add("product3", A("product", a, b, e))
    add("median5", A("median", a, b, e, f, g))
    add("median5_mm", A("median", a, b, e, f, g, mm=-9, dv=4))
    add("median2", A("median", a, b))
    add("and2", A("and", a, b))
    add("or2", A("or", a, b))
    add("and_mm", A("and", a, b, mm=0.5))
    add("or_mm", A("or", a, b, mm=-0.5))
    add("and3", A("and", a, b, A("not", e)))
    add("if3", A("if", a, b, e))
    add("if2", A("if", a, b))
    add("if3_dv", A("if", a, b, e, mm=5, dv=7))  # neither attribute applies to ``if``
    add("if_cmp", A("if", A("lessThan", a, b), A("*", a, K(2)), A("*", b, K(-0.5))))
    add("if_in_dv", A("+", A("if", a, b, e), K(0), mm=-6, dv=6))  # a missing taken branch under an outer default
    add("ismiss", A("isMissing", a))
    add("isnotmiss", A("isNotMissing", b))
    add("mm_ref", A("+", R("a", mm=1.5), R("b", mm=-2)))
    add("both_missing_in", A("-", a, b, mm=11, dv=13))
    add("both_nan_result", A("*", a, b, mm=11, dv=13))  # 0 * inf and inf - inf: NaN from present inputs
    add("both_inf_result", A("/", a, K(0), mm=11, dv=13))  # x / 0: an infinity is not replaced; 0 / 0 is
    add("trunc", A("+", a, K(0)), "integer")
    add("trunc_b", A("*", b, K(1)), "integer")
    add("float_field", A("*", a, K(0.5)), "float")
    add("over", A("+", a, a))  # FLT_MAX + FLT_MAX: an infinity in fp32
    add("under", A("*", a, K(0.125)))  # 2^-152: a signed zero in fp32
    add("sub_keep", A("*", a, K(4)))  # 2^-147: a subnormal that keeps its bits
    add("isin_num", A("isIn", a, K(1), K(-0.0), K(2.5), K(BIG_INT)))
    add("isnotin_num", A("isNotIn", b, K(0.5), K(-2.25), mm=3))
    add("isin_str", A("isIn", R("c"), K("red"), K("blue"), mm=-1))
    add("isnotin_str", A("isNotIn", R("c"), K("green")))
    return F


def norm_fields() -> List[tuple]:
    F: List[tuple] = []

    def add(name, body, dtype="double"):
        F.append((name, dtype, body))

    for nm, knots in (("k2", KNOTS2), ("k3", KNOTS3), ("k5", KNOTS5)):
        for outl in ("asIs", "asMissingValues", "asExtremeValues"):
            add(f"nc_{nm}_{outl}", NC("a", knots, outl))
            add(f"nc_{nm}_{outl}_mm", NC("a", knots, outl, mm=-7.5))
    return F


def table_fields() -> List[tuple]:
    """NormDiscrete, Discretize, MapValues and string copies: no arithmetic, so no row is ever inexact
    and every special input stays in the table."""
    F: List[tuple] = []

    def add(name, body, dtype="double"):
        F.append((name, dtype, body))

    add("nd_red", ND("c", "red"))
    add("nd_blue_mm", ND("c", "blue", mm=-1))
    add("nd_num", ND("b", "2", mm=0.5))
    shared = (("1", "closedClosed", -1.0, 1.0), ("2", "openOpen", 1.0, 2.0), ("3", "closedOpen", 2.0, 3.0),
              ("4", "openClosed", 3.0, 4.0))
    add("dz_closures", DZ("a", shared, mm=-1, dv=9))
    add("dz_closures_rev", DZ("a", (("4", "openClosed", 1.0, 2.0), ("3", "closedOpen", 0.0, 1.0),
                                    ("2", "openOpen", -1.0, 0.0), ("1", "closedClosed", -2.0, -1.0)), dv=0))
    add("dz_overlap", DZ("a", (("1", "closedClosed", 0.0, 2.0), ("2", "closedClosed", 1.0, 3.0),
                               ("3", "openOpen", -1.0, 8.0)), dv=-2))
    add("dz_gap", DZ("a", (("1", "closedOpen", -4.0, -2.0), ("2", "openClosed", 0.5, 4.0)), mm=7, dv=5))
    add("dz_gap_nodefault", DZ("a", (("1", "closedOpen", -4.0, -2.0), ("2", "openClosed", 0.5, 4.0))))
    add("dz_unbounded", DZ("a", (("-1", "openOpen", None, -1.0), ("0", "closedClosed", -1.0, 1.0),
                                 ("1", "openClosed", 1.0, None))))
    add("dz_string", DZ("a", (("low", "openOpen", None, 0.0), ("mid", "closedClosed", 0.0, 2.0),
                              ("high", "openOpen", 2.0, None)), mm="none"), "string")
    add("dz_string_read", MV(["dz_string"], (("low", "-1.5"), ("mid", "0.25"), ("high", "2.5"), ("none", "8")), dv=99))
    add("mv1", MV(["c"], (("red", "1.5"), ("blue", "-2"), ("red", "77")), mm=-1, dv=0.5))  # a duplicate key: the first wins
    add("mv1_bare", MV(["c"], (("green", "4"),)))
    add("mv2", MV(["c", "b"], (("red", "1", "10"), ("red", "2", "20"), ("green", "1", "30"), ("red", "1", "40"),
                               ("blue", "3", "-0.0")), mm=-5, dv=-0.5))
    add("mv3", MV(["c", "b", "c2"], (("red", "1", "red", "1"), ("red", "1", "green", "2"), ("green", "2", "blue", "3"),
                                     ("blue", "1", "blue", "4"), ("red", "2", "red", "5"), ("green", "1", "red", "6")), dv=0))
    add("copy", R("c"), "string")  # string-to-string field copy: REMAP
    add("copy_mm", R("c2"), "string")
    add("copy_read", MV(["copy", "copy_mm"], tuple((x, y, str(3 * i + j + 1)) for i, x in enumerate(COLOURS)
                                                   for j, y in enumerate(COLOURS)), mm=-1, dv=-2))
    add("num_key", MV(["b"], (("1", "0.125"), ("2", "-0.25"), ("2", "3")), dv=-4))
    return F


def chain_fields() -> List[tuple]:
    a, b = R("a"), R("b")
    return [
        ("h1", "double", A("*", a, K(0.5))),                       # read by h2 and h3
        ("h2", "double", A("+", R("h1"), b)),
        ("h3", "double", A("-", R("h1"), K(0.25))),
        ("h4", "double", A("max", R("h2"), R("h3"), R("h1"))),     # depth 3
        ("h5", "double", NC("h4", KNOTS3, "asExtremeValues", mm=-1)),  # depth 4
        ("t1", "integer", A("+", a, K(0))),                       # truncated, then read
        ("t2", "double", A("-", a, R("t1"))),                      # the fraction that was cut off
        ("z1", "double", A("min", a, b)),                          # a signed zero carried through a column
        ("z2", "double", A("if", A("equal", R("z1"), K(0)), A("/", K(1), R("z1")), R("z1"))),
        ("s1", "string", DZ("a", (("neg", "openOpen", None, 0.0), ("pos", "closedOpen", 0.0, None)), mm="none")),
        ("s2", "string", R("s1")),
        ("s3", "double", MV(["s2"], (("neg", "-1"), ("pos", "1"), ("none", "0.5")))),
    ]


CHAIN_SELECTED = ("h2", "h3", "h4", "h5", "t1", "t2", "z2", "s3", "h1")


def stack_expr(depth: int) -> str:
    """``a + (a + (... + b))``: every level keeps one operand on the stack, ``depth`` slots at the bottom."""
    body = R("b")
    for _ in range(depth - 1):
        body = A("+", R("a"), body)
    return body


def wide_fields(n_derived: int) -> List[tuple]:
    """Cheap exact columns that depend on their index (a transposed or shifted column shows)."""
    out = []
    for j in range(n_derived):
        kind = j % 4
        if kind == 0:
            body = A("+", R("a"), K(j / 8.0))
        elif kind == 1:
            body = A("*", R("b"), K(float(j % 16 - 8)))
        elif kind == 2:
            body = A("threshold", R("a"), K((j % 128 - 64) / 8.0))
        else:
            body = A("-", R(f"w{j - 3}"), R("c"), mm=float(j))
        out.append((f"w{j}", "double", body))
    return out


PREP_LOW, PREP_HIGH = -2.0, 3.0


def prep_document() -> str:
    fields = [("p1", "double", A("+", R("a"), R("b"))), ("p2", "double", A("*", R("e"), K(2))),
              ("p3", "double", A("isMissing", R("a")))]
    return document(
        ("a", "b", "e"), fields, ("p1", "p2", "p3", "b"),
        data_attrs={"e": '<Interval closure="closedOpen" leftMargin="-1" rightMargin="5"/>'},
        mining_attrs={"a": ' missingValueReplacement="0.75"',
                      "b": f' outliers="asExtremeValues" lowValue="{num(PREP_LOW)}" highValue="{num(PREP_HIGH)}"',
                      "e": ' invalidValueTreatment="returnInvalid"'})


def prep_table(n: int = 300):
    """``(X, P, ok)``: raw rows, the prepared matrix and row validity, by construction. Invalid rows
    (e outside [-1, 5)) sit in the first and in the last workgroup, and valid rows in both."""
    X = _grid_rows(n, 3, seed=31)
    X[:, 2] = np.clip(np.nan_to_num(X[:, 2]), -1.0, 4.875)
    X[::9, 0] = NAN
    X[4, 1], X[5, 1], X[6, 1], X[7, 1] = PREP_LOW, PREP_HIGH, -INF, INF
    X[8, 1] = NAN
    bad = {3: -1.125, 100: 5.0, 127: INF, n - 2: -8.0, n - 41: 5.125}
    for r, v in bad.items():
        X[r, 2] = v
    X[n - 1, 2] = NAN  # a missing value is not invalid
    X[9, 2], X[10, 2] = -1.0, float(np.nextafter(F32(5.0), F32(0.0)))
    P = X.copy()
    P[np.isnan(P[:, 0]), 0] = 0.75
    P[:, 1] = np.where(P[:, 1] < PREP_LOW, PREP_LOW, np.where(P[:, 1] > PREP_HIGH, PREP_HIGH, P[:, 1]))
    ok = np.ones(n, bool)
    ok[list(bad)] = False
    return X, P, ok


# --------------------------------------------------------------------------- cases


class Case:
    """One document with its table. ``X`` raw fp32 rows, ``P`` / ``ok`` the prepared matrix and row
    validity, ``ref`` the fp32 reference columns of ``prog.selected``, ``claims`` the populations the
    case places (name -> row mask), ``margins`` the midpoint margins (rounded family)."""

    def __init__(self, name: str, doc: str, X: np.ndarray, family: str = "exact", P=None, ok=None, drop: bool = True):
        from flink_jpmml_amd.runtime.compiled import CompiledPmml
        from flink_jpmml_amd.runtime.derive import plan_field_layout

        self.name, self.doc, self.family = name, doc, family
        self.c = CompiledPmml.from_string(doc)
        layout = plan_field_layout(self.c)
        assert layout.program is not None, name
        self.prog = layout.program
        X = np.asarray(X, F32).astype(np.float64)
        assert X.shape[1] == len(self.c.active_fields)
        if P is None:  # no preparation: the kernel sees the raw rows
            P, ok = X, np.ones(len(X), bool)
        ref = Reference(self.c)
        cols = ref.columns(P, self.prog.selected, rounded=family == "rounded")
        self.dropped = 0
        if family == "exact":  # rows this document cannot hold exactly: an inexact float64 intermediate, or a
            keep = ~ref.inexact  # rounded fp32 value in a column that another field reads
            keep[[r for _, r in ref.inexact_read]] = False
            self.dropped = int((~keep).sum())
            if self.dropped and drop:
                X, P, ok = X[keep], P[keep], ok[keep]
                cols = ref.columns(P, self.prog.selected)
                assert not ref.inexact.any() and not ref.inexact_read, name  # the guard: a bad probe fails here
        self.X, self.P, self.ok, self.ref = X.astype(F32), P, ok, cols
        self.inexact, self.inexact_read, self.rounded_store = ref.inexact, ref.inexact_read, ref.rounded_store
        self.margins = ref.margins
        self.claims: Dict[str, np.ndarray] = {}
        for arr in (self.X, self.P, self.ok, self.ref):
            arr.setflags(write=False)

    def col(self, name: str) -> np.ndarray:
        return self.ref[:, self.prog.selected.index(name)]

    def oracle(self) -> np.ndarray:
        """The float64 oracle's columns, rounded to fp32."""
        cols = self.c.columns(self.P)
        with np.errstate(over="ignore"):
            return np.stack([cols.get(nm).astype(F32) for nm in self.prog.selected], axis=1)

    def twin(self, mutant: str = ""):
        return twin(self.prog, self.P, self.ok, mutant)


def _numeric(fields) -> List[str]:
    return [nm for nm, dtype, _ in fields if dtype != "string"]


def _col_has(X: np.ndarray, j: int, s: float) -> np.ndarray:
    if s != s:
        return np.isnan(X[:, j])
    return (X[:, j] == s) & (np.signbit(X[:, j]) == (math.copysign(1.0, s) < 0))


@functools.lru_cache(maxsize=None)
def apply_case() -> Case:
    fields = apply_fields()
    case = Case("apply", document(tuple("abefg") + ("c",), fields, _numeric(fields), strings=("c",)), apply_table())
    X = case.X.astype(np.float64)
    a, b, e = X[:, 0], X[:, 1], X[:, 2]
    cl = case.claims
    for j, f in enumerate("abefg"):
        for s, nm in zip(SPECIALS, ("+0", "-0", "nan", "subnormal", "flt-min", "flt-max", "2^24+2", "+inf", "-inf")):
            cl[f"special {nm} in {f}"] = _col_has(X, j, s)
    for s, nm in ((0.0, "+0"), (-0.0, "-0"), (NAN, "nan")):
        cl[f"special {nm} in c"] = _col_has(X, 5, s)
    cl["store: above FLT_MAX becomes inf"] = np.isinf(case.col("over")) & np.isfinite(a)
    cl["store: below the subnormals becomes +0"] = (a == FLT_SUB) & (bits(case.col("under")) == 0)
    cl["store: below the subnormals becomes -0"] = (a == -0.0) & np.signbit(a) & (bits(case.col("under")) == 0x80000000)
    cl["store: a subnormal keeps its bits"] = (a == FLT_SUB) & (bits(case.col("sub_keep")) == 4)
    for v in (-0.5, -1.5, 2.5):
        cl[f"integer store truncates {v}"] = (a == v) & (case.col("trunc") == math.trunc(v))
    cl["integer store of -0.5 is -0"] = (a == -0.5) & (bits(case.col("trunc")) == 0x80000000)
    cl["integer store leaves NaN"] = np.isnan(a) & np.isnan(case.col("trunc"))
    for k in range(-4, 5):
        cl[f"round / rint at {k + 0.5}"] = a == k + 0.5
    cl["round and rint differ"] = bits(case.col("u_round")) != bits(case.col("u_rint"))
    fin = np.isfinite(a) & np.isfinite(b) & (b != 0)
    for sa in (1, -1):
        for sb in (1, -1):
            cl[f"modulo signs {sa} {sb}"] = fin & (a * sa > 0) & (b * sb > 0) & (case.col("mod") != 0)
    cl["modulo zero result, b > 0"] = fin & (b > 0) & (bits(case.col("mod")) == 0) & (a != 0)
    cl["modulo zero result, b < 0 is -0"] = fin & (b < 0) & (bits(case.col("mod")) == 0x80000000) & (a != 0)
    cl["modulo zero shows as -inf"] = fin & (case.col("mod_inv") == -INF)
    cl["modulo b = 0"] = (b == 0) & ~np.isnan(a) & np.isnan(case.col("mod"))
    cl["modulo a = +-inf"] = np.isinf(a) & np.isfinite(b) & (b != 0) & np.isnan(case.col("mod"))
    cl["modulo b = +-inf"] = np.isinf(b) & np.isfinite(a)
    cl["modulo b = +-inf, other sign"] = np.isinf(b) & np.isfinite(a) & np.isinf(case.col("mod"))
    neg0 = lambda v: (v == 0) & np.signbit(v)  # noqa: E731
    pos0 = lambda v: (v == 0) & ~np.signbit(v)  # noqa: E731
    cl["min / max of (-0, +0)"] = neg0(a) & pos0(b) & (case.col("min2_inv") == -INF) & (case.col("max2_inv") == INF)
    cl["min / max of (+0, -0)"] = pos0(a) & neg0(b) & (case.col("min2_inv") == -INF) & (case.col("max2_inv") == INF)
    five = X[:, :5]
    present = (~np.isnan(five)).sum(axis=1)
    for k in range(6):
        cl[f"aggregates with {k} of 5 present"] = present == k
    srt = np.sort(np.where(np.isnan(five), INF, five), axis=1)
    cl["aggregates with duplicates"] = (present >= 3) & (srt[:, 1:3] == srt[:, 0:2]).any(axis=1)
    cl["aggregates in descending order"] = (present == 5) & (five[:, 1:] < five[:, :-1]).all(axis=1)
    for cond, nm in ((1.0, "1"), (0.0, "+0"), (2.0, "2"), (-0.0, "-0"), (NAN, "missing")):
        cl[f"if condition {nm}"] = _col_has(X, 0, cond)
    cl["if: missing taken branch"] = (a == 1.0) & np.isnan(b) & np.isnan(case.col("if3_dv"))
    cl["if: missing taken branch under an outer defaultValue"] = (a == 1.0) & np.isnan(b) & (case.col("if_in_dv") == -6)
    cl["if with two arguments, condition 0"] = (a == 0.0) & np.isnan(case.col("if2"))
    cl["and / or with a missing argument"] = (np.isnan(a) ^ np.isnan(b)) & np.isnan(case.col("and2"))
    cl["and / or with a missing argument and mapMissingTo"] = (np.isnan(a) ^ np.isnan(b)) & (case.col("and_mm") == 0.5)
    cl["-0.0 == 0.0"] = neg0(a) & pos0(b) & (case.col("c_equal") == 1)
    cl["equal values reached by different arithmetic"] = (case.col("eq_arith") == 1) & (a != 0)
    cl["mapMissingTo and defaultValue: a missing input"] = np.isnan(a) & (case.col("both_missing_in") == 11)
    cl["mapMissingTo and defaultValue: NaN from present inputs"] = ~np.isnan(a) & ~np.isnan(b) & (case.col("both_nan_result") == 13)
    cl["mapMissingTo and defaultValue: 0 / 0"] = (a == 0) & (case.col("both_inf_result") == 13)
    cl["mapMissingTo and defaultValue: an infinite result stays"] = np.isfinite(a) & np.isinf(case.col("both_inf_result"))
    cl["isIn on a numeric field, missing input"] = np.isnan(a) & np.isnan(case.col("isin_num"))
    cl["isIn on a numeric field, a member"] = case.col("isin_num") == 1
    cl["isIn on a string field, missing input"] = np.isnan(X[:, 5]) & (case.col("isin_str") == -1)
    cl["isNotIn on a string field"] = case.col("isnotin_str") == 1
    return case


@functools.lru_cache(maxsize=None)
def norm_case() -> Case:
    fields = norm_fields()
    case = Case("norm", document(("a", "b", "c", "c2"), fields, _numeric(fields), strings=("c", "c2")), norm_table())
    X = case.X.astype(np.float64)
    a = X[:, 0]
    cl = case.claims
    for nm, knots in (("k2", KNOTS2), ("k3", KNOTS3), ("k5", KNOTS5)):
        for o, _ in knots:
            o32 = F32(o)
            cl[f"{nm}: on knot {o}"] = a == o
            cl[f"{nm}: one ulp below knot {o}"] = a == float(np.nextafter(o32, F32(-INF)))
            cl[f"{nm}: one ulp above knot {o}"] = a == float(np.nextafter(o32, F32(INF)))
        for outl in ("asIs", "asMissingValues", "asExtremeValues"):
            cl[f"{nm} {outl}: below the first knot"] = a < knots[0][0]
            cl[f"{nm} {outl}: above the last knot"] = a > knots[-1][0]
        cl[f"{nm}: missing with mapMissingTo"] = np.isnan(a) & (case.col(f"nc_{nm}_asIs_mm") == -7.5)
        cl[f"{nm}: missing without"] = np.isnan(a) & np.isnan(case.col(f"nc_{nm}_asIs"))
    cl["a decreasing norm"] = (a > -2) & (a < 5) & (case.col("nc_k5_asIs") < 6)
    return case


@functools.lru_cache(maxsize=None)
def table_case() -> Case:
    fields = table_fields()
    case = Case("table", document(("a", "b", "c", "c2"), fields, _numeric(fields), strings=("c", "c2")), norm_table())
    X = case.X.astype(np.float64)
    a = X[:, 0]
    cl = case.claims
    for s, nm in zip(SPECIALS, ("+0", "-0", "nan", "subnormal", "flt-min", "flt-max", "2^24+2", "+inf", "-inf")):
        cl[f"special {nm} in a"] = _col_has(X, 0, s)
    cl["Discretize: overlapping bins, the first wins"] = (a >= 1) & (a <= 2) & (case.col("dz_overlap") == 1)
    cl["Discretize: a gap takes the default"] = (a >= -2) & (a <= 0.5) & (case.col("dz_gap") == 5)
    cl["Discretize: a gap without a default"] = (a >= -2) & (a <= 0.5) & np.isnan(case.col("dz_gap_nodefault"))
    cl["Discretize: unbounded below"] = (a == -INF) & (case.col("dz_unbounded") == -1)
    cl["Discretize: unbounded above"] = (a == INF) & (case.col("dz_unbounded") == 1)
    for edge in (1.0, 2.0, 3.0):
        cl[f"Discretize: shared edge {edge}"] = a == edge
    cl["Discretize: string output"] = case.col("dz_string_read") == 2.5
    cl["Discretize: string output, missing"] = np.isnan(a) & (case.col("dz_string_read") == 8)
    cl["MapValues 1 key: duplicate row, the first wins"] = (X[:, 2] == 0) & (case.col("mv1") == 1.5)
    cl["MapValues 1 key: missing"] = np.isnan(X[:, 2]) & (case.col("mv1") == -1)
    cl["MapValues 1 key: no match with a default"] = (X[:, 2] == 1) & (case.col("mv1") == 0.5)
    cl["MapValues 1 key: no match without"] = (X[:, 2] != 1) & ~np.isnan(X[:, 2]) & np.isnan(case.col("mv1_bare"))
    cl["MapValues 2 keys: a match"] = case.col("mv2") == 20
    cl["MapValues 2 keys: duplicate row"] = (X[:, 2] == 0) & (X[:, 1] == 1) & (case.col("mv2") == 10)
    cl["MapValues 2 keys: one key missing"] = (np.isnan(X[:, 2]) ^ np.isnan(X[:, 1])) & (case.col("mv2") == -5)
    cl["MapValues 2 keys: first key matches, second does not"] = (X[:, 2] == 0) & (X[:, 1] == 3) & (case.col("mv2") == -0.5)
    cl["MapValues 3 keys: a match on a later row"] = case.col("mv3") == 6
    cl["MapValues 3 keys: one key missing, no mapMissingTo"] = np.isnan(X[:, 3]) & ~np.isnan(X[:, 2]) & np.isnan(case.col("mv3"))
    cl["REMAP: string copies"] = case.col("copy_read") == 6
    cl["REMAP: missing source"] = np.isnan(X[:, 2]) & (case.col("copy_read") == -1)
    cl["REMAP: both sources present"] = (X[:, 3] == 1) & (X[:, 2] == 2) & (case.col("copy_read") == 8)
    return case


@functools.lru_cache(maxsize=None)
def chain_case() -> Case:
    T = apply_table()[:, :2]
    case = Case("chain", document(("a", "b"), chain_fields(), CHAIN_SELECTED), T)
    a = case.X[:, 0].astype(np.float64)
    case.claims["a derived field read by two later ones"] = ~np.isnan(case.col("h2")) & ~np.isnan(case.col("h3"))
    case.claims["a chain of depth 4"] = ~np.isnan(case.col("h5")) & (case.col("h5") != -1)
    case.claims["a truncated column read back"] = case.col("t2") == 0.5
    case.claims["a signed zero read back from a column"] = case.col("z2") == -INF
    case.claims["a string column copied and read"] = (case.col("s3") == -1) & (a < 0)
    return case


@functools.lru_cache(maxsize=None)
def fp32_column_case() -> Case:
    """Finding 2: ``d1 = a / 3`` is an fp32 column on the device; ``d2`` reads it."""
    fields = [("d1", "double", A("/", R("a"), K(3))), ("d2", "double", A("greaterThan", A("*", R("d1"), K(3)), R("a"))),
              ("d3", "double", A("-", A("*", R("d1"), K(3)), R("a")))]
    vals = np.concatenate([GRID, np.arange(1, 200.0), [NAN, 0.0, -0.0, INF, FLT_MAX, FLT_MIN, BIG_INT]])
    return Case("fp32-column", document(("a",), fields, ("d2", "d3", "d1")), vals[:, None], family="ieee")


@functools.lru_cache(maxsize=None)
def stack_case() -> Case:
    T = _grid_rows(300, 2, seed=41)
    return Case("stack-16", document(("a", "b"), [("deep", "double", stack_expr(16))], ("deep",)), T)


def stack_document(depth: int) -> str:
    return document(("a", "b"), [("deep", "double", stack_expr(depth))], ("deep",))


def chained_fields(n_derived: int) -> List[tuple]:
    """Every column reads the one before it, so selecting the last alone keeps them all in the tile."""
    out = [("w0", "double", A("+", R("a"), R("c"), mm=0.5))]
    for j in range(1, n_derived):
        out.append((f"w{j}", "double", A("+", R(f"w{j - 1}"), K(((5 * j) % 9 - 4) / 8.0))))
    return out


def wide_document(n_tile: int, n_select: int = 0) -> str:
    """``n_select`` 0: every tile column is selected (the regression kernel behind holds 128 at most);
    otherwise a chain of ``n_tile`` - 3 fields of which the last ``n_select`` are."""
    fields = chained_fields(n_tile - 3) if n_select else wide_fields(n_tile - 3)
    names = [nm for nm, _, _ in fields]
    return document(("a", "b", "c"), fields, names[-n_select:] if n_select else ["a", "b", "c"] + names)


@functools.lru_cache(maxsize=None)
def wide_case(n_tile: int) -> Case:
    T = _grid_rows(300, 3, seed=50 + n_tile)
    T[:, 2] = np.round(T[:, 2])
    return Case(f"wide-{n_tile}", wide_document(n_tile, 128 if n_tile > 128 else 0), T)


@functools.lru_cache(maxsize=None)
def prep_case() -> Case:
    X, P, ok = prep_table()
    case = Case("prep", prep_document(), X, P=P, ok=ok)
    n = len(X)
    first, last = np.arange(n) < DTB, np.arange(n) >= (n - 1) // DTB * DTB
    case.claims["row_ok 0 in the first workgroup"] = ~case.ok & first
    case.claims["row_ok 1 in the first workgroup"] = case.ok & first
    case.claims["row_ok 0 in the last workgroup"] = ~case.ok & last
    case.claims["row_ok 1 in the last workgroup"] = case.ok & last
    case.claims["missingValueReplacement applied"] = np.isnan(X[:, 0]) & (case.col("p3") == 0)
    case.claims["outliers clamped"] = (X[:, 1] != P[:, 1]) & ~np.isnan(X[:, 1])
    return case


def _nudge_rounded(X: np.ndarray, fields) -> np.ndarray:
    """Replace probe inputs whose value falls within 2^-40 of an fp32 midpoint under any function."""
    X = X.copy()
    for r in range(len(X)):
        for _ in range(8):
            a, b = float(X[r, 0]), float(X[r, 1])
            if a != a:
                break
            unary = min(rounded_value(fn, a)[1] for fn in ROUNDED_UNARY)
            binary = min(rounded_value(fn, a, b)[1] for fn in ROUNDED_BINARY) if b == b else INF
            if unary <= MID_REL:  # sqrt(2^24 + 2) is 2^-49 from the midpoint above 4096: 2^24 + 2 moves on
                X[r, 0] = float(F32(a * 0.9921875))
            elif binary <= MID_REL:  # 2^-149 / 2 is the midpoint between 0 and 2^-149: the divisor moves on
                X[r, 1] = b + 1.0
            else:
                break
    return X


def rounded_fields() -> List[tuple]:
    F = [("r_" + fn, "double", A(fn, R("a"))) for fn in ROUNDED_UNARY]
    F += [("r_" + {"/": "div"}.get(fn, fn), "double", A(fn, R("a"), R("b"))) for fn in ROUNDED_BINARY]
    F += [("r_ln_dv", "double", A("ln", R("a"), mm=-1, dv=-2)), ("r_sqrt_dv", "double", A("sqrt", R("a"), mm=-1, dv=-2)),
          ("r_div_dv", "double", A("/", R("a"), R("b"), mm=-1, dv=-2))]
    return F


@functools.lru_cache(maxsize=None)
def rounded_case() -> Case:
    fields = rounded_fields()
    X = _nudge_rounded(rounded_table(), fields)
    case = Case("rounded", document(("a", "b"), fields, _numeric(fields)), X, family="rounded")
    a, b = case.X[:, 0].astype(np.float64), case.X[:, 1].astype(np.float64)
    cl = case.claims
    cl["exact: sqrt 4"] = (a == 4) & (case.col("r_sqrt") == 2)
    cl["exact: exp 0"] = (a == 0) & (case.col("r_exp") == 1)
    cl["exact: log10 100"] = (a == 100) & (case.col("r_log10") == 2)
    cl["exact: pow(2, 3)"] = (a == 2) & (b == 3) & (case.col("r_pow") == 8)
    cl["exact: hypot(3, 4)"] = (a == 3) & (b == 4) & (case.col("r_hypot") == 5)
    for v in (-1, -4, -6, -8, -8.5, -10, -13, 0, 8.5):
        cl[f"stdNormalCDF at {v}"] = (a == v) & ~np.isnan(case.col("r_stdNormalCDF"))
    cl["stdNormalCDF lower tail is not zero"] = (a == -8.5) & (case.col("r_stdNormalCDF") > 0)
    cl["ln(-1) takes the default"] = (a == -1) & (case.col("r_ln_dv") == -2)
    cl["sqrt(-1) takes the default"] = (a == -1) & (case.col("r_sqrt_dv") == -2)
    cl["0 / 0 takes the default"] = (a == 0) & (b == 0) & (case.col("r_div_dv") == -2)
    cl["x / 0 stays infinite"] = (a != 0) & (b == 0) & np.isinf(case.col("r_div_dv"))
    cl["sin(-0.0) keeps the sign"] = (a == 0) & np.signbit(a) & (bits(case.col("r_sin")) == 0x80000000)
    return case


def plan_cases() -> List[Case]:
    """The documents that run through ``DerivedPlan.launch`` at every row count."""
    return [apply_case(), norm_case(), table_case(), chain_case(), fp32_column_case(), stack_case(), prep_case(), rounded_case(),
            wide_case(95), wide_case(96), wide_case(256), n_sel_one_case()]


@functools.lru_cache(maxsize=None)
def n_sel_one_case() -> Case:
    T = _grid_rows(300, 3, seed=61)
    T[:, 2] = np.round(T[:, 2])
    return Case("wide-96-one-selected", wide_document(96, n_select=1), T)


# --------------------------------------------------------------------------- direct launch harness

LAYOUTS = ("contiguous", "ldx-multiple-of-4", "odd-ldx", "misaligned-base", "aligned-n-in-not-multiple-of-4")


def lay_out(X: np.ndarray, layout: str):
    """``(flat fp32 buffer, offset, ldx)``: the rows of ``X`` at ``buffer[offset + r * ldx + j]``, every other
    element 97 (a value no probe expects). The offset counts floats past a 16-byte aligned base."""
    n, k = X.shape
    up4 = (k + 3) // 4 * 4
    off, ldx = {"contiguous": (0, k), "ldx-multiple-of-4": (0, up4 + 4), "odd-ldx": (0, (k + 2) | 1),
                "misaligned-base": (1, up4 + 4), "aligned-n-in-not-multiple-of-4": (0, up4 + 4)}[layout]
    if layout == "aligned-n-in-not-multiple-of-4":
        assert k % 4 != 0
    buf = np.full(off + n * ldx + 8, 97.0, F32)
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(n, k), strides=(4 * ldx, 4))
    view[:] = X
    return buf, off, ldx


def launch_direct(plan, X: np.ndarray, layout: str = "contiguous", stream=None):
    """``pmml_derive_launch`` through ctypes with ``ops/_lib.DeriveArgs`` on the plan's own program.
    ``out`` and ``row_ok`` carry ``GUARD`` sentinel elements before and after. Returns ``(cols fp32
    [rows, n_sel], row_ok uint8, guards)``; the guards must all still hold the sentinel."""
    import ctypes

    import torch

    from flink_jpmml_amd.ops._lib import DeriveArgs, ptr, stream_handle

    n = len(X)
    buf, off, ldx = lay_out(np.asarray(X, F32), layout)
    dev = plan.device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        xb = torch.from_numpy(buf).to(dev)
        assert xb.data_ptr() % 16 == 0
        out = torch.full((GUARD + n * plan.n_sel + GUARD,), SENTINEL32, dtype=torch.int32, device=dev)
        rok = torch.full((GUARD + n + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
        a = DeriveArgs()
        a.X = xb.data_ptr() + 4 * off
        a.n_rows, a.n_in, a.ldx, a.n_tile = n, X.shape[1], ldx, plan.n_tile
        a.prep, a.prog, a.pool, a.out_cols = ptr(plan.prep), ptr(plan.insns), ptr(plan.pool), ptr(plan.out_cols)
        a.n_insn, a.n_sel = plan.n_insn, plan.n_sel
        a.out, a.row_ok = out.data_ptr() + 4 * GUARD, rok.data_ptr() + GUARD
        rc = plan.lib.pmml_derive_launch(stream_handle(s), ctypes.byref(a))
        assert rc == 0, rc
    s.synchronize()
    out_h, rok_h = out.cpu().numpy(), rok.cpu().numpy()
    cols = out_h[GUARD: GUARD + n * plan.n_sel].view(F32).reshape(n, plan.n_sel)
    guards = {"out before": out_h[:GUARD], "out after": out_h[GUARD + n * plan.n_sel:],
              "row_ok before": rok_h[:GUARD], "row_ok after": rok_h[GUARD + n:]}
    return cols, rok_h[GUARD: GUARD + n], guards


def assert_guards(guards: dict) -> None:
    for nm, g in guards.items():
        want = 0x5A if g.dtype == np.uint8 else SENTINEL32
        assert (g == want).all(), f"guard elements of {nm} were written"
