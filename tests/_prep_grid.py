"""The field-preparation grid of the boundary tests: one MiningField / DataField treatment per
document (CPU twin test) or per column (GPU tests), with the inputs that sit on its bounds.

A treatment is ``(name, DataField children, DataField dataType or None, MiningField attributes,
bounds, safe)``; ``bounds`` are the constants its comparisons use, ``safe`` a valid ordinary value
(the other columns of a row that probes one column hold it). Each is crossed with every
``invalidValueTreatment``, with ``dataType`` float and double, and with a bound fp32 rounds up
(0.3 -> 0.300000012) and one it rounds down (0.7 -> 0.699999988)."""

import re
from typing import List, Optional, Tuple

import numpy as np

from tests._boundary import F32, around

BOUNDS = {"up": 0.3, "down": 0.7}  # fp32(0.3) > 0.3, fp32(0.7) < 0.7
CLOSURES = ["closedClosed", "openOpen", "closedOpen", "openClosed"]
INVALID_TREATMENTS = ["returnInvalid", "asMissing", "asIs", "asValue"]
DTYPES = ["float", "double"]
INVALID_REPL = -0.25   # fp32-exact replacements: the prepared value is the same number in both
MISSING_REPL = 0.125
INT_INVALID_REPL = -2
INT_MISSING_REPL = 1
SENT = -999.0


def families(b: float) -> dict:
    """Treatment families over the bound ``b``: name -> list of (case name, DataField children,
    dataType override, extra MiningField attributes, bounds whose neighbourhood is probed, safe value)."""
    iv_left = [(f"left-{c}", f'<Interval closure="{c}" leftMargin="{b}" rightMargin="5"/>', None, "", [b, 5.0], 1.0)
               for c in CLOSURES]
    iv_right = [(f"right-{c}", f'<Interval closure="{c}" leftMargin="-5" rightMargin="{b}"/>', None, "", [b, -5.0], -1.0)
                for c in CLOSURES]
    outl = [(f"{kind}-{side}", "", None, f'outliers="{kind}" {side}Value="{b}"', [b], 1.0 if side == "low" else -1.0)
            for kind in ("asMissingValues", "asExtremeValues") for side in ("low", "high")]
    sentinel = '<Value value="-999" property="missing"/>'
    lists = [
        ("sentinel", sentinel, None, "", [SENT], 0.25),
        ("sentinel-interval", sentinel + f'<Interval closure="closedOpen" leftMargin="-1000" rightMargin="{b}"/>',
         None, "", [SENT, b, -1000.0], -1.0),
        ("lists", sentinel + '<Value value="-7" property="missing"/><Value value="0.5" property="invalid"/>'
         '<Value value="2" property="invalid"/>', None, "", [SENT, -7.0, 0.5, 2.0], 0.25),
        ("lists-interval", sentinel + '<Value value="-7" property="missing"/><Value value="0.5" property="invalid"/>'
         f'<Value value="2" property="invalid"/><Interval closure="closedClosed" leftMargin="-1" rightMargin="{b + 1}"/>',
         None, "", [SENT, -7.0, 0.5, 2.0, -1.0, b + 1], 0.25),
        ("invalid-interval", f'<Value value="0.5" property="invalid"/><Interval closure="closedClosed" leftMargin="-1" '
         f'rightMargin="{b + 1}"/>', None, "", [0.5, -1.0, b + 1], 0.25),
    ]
    integer = [("integer", "", "integer", "", [3.0, -3.0, 0.0, 2.0 ** 24, -2.0 ** 24, 2.0 ** 23 - 1], 1.0)]
    return {"interval-left": iv_left, "interval-right": iv_right, "outliers": outl, "lists": lists,
            "integer": integer}


def mask_cases() -> list:
    """Numeric categories as a 64-bit value mask (``FP_VALUE_MASK``): valid values lo, lo + 63 and
    a few between; lo - 1 and lo + 64 are outside the mask's span."""
    lo = 10
    vals = [lo, lo + 1, lo + 31, lo + 32, lo + 62, lo + 63]
    kids = "".join(f'<Value value="{v}"/>' for v in vals)
    return [("mask", kids, "integer", "", [float(v) for v in (lo - 1, lo, lo + 1, lo + 2, lo + 31, lo + 32, lo + 33,
                                                               lo + 62, lo + 63, lo + 64)], float(lo + 1))]


def probe_values(bounds: List[float]) -> np.ndarray:
    """Every bound +-{0, 1, 2} ulps, +-inf, NaN (fp32)."""
    return np.concatenate([around(bounds), np.array([np.inf, -np.inf, np.nan], dtype=F32)])


def treat_field(txt: str, j: int, children: str, data_type: Optional[str], attrs: str, dtype: str,
                invalid_treatment: str) -> str:
    """Apply one treatment to field ``f<j>`` of a ``bench/synth.py`` document. A list of valid
    ``<Value>``s makes the field categorical (numeric categories); an integer field takes integer
    replacements (others would make the document invalid)."""
    name = f"f{j}"
    categorical = "<Value value" in children and "property=" not in children
    integer = (data_type or dtype) == "integer"
    m = re.search(rf'<DataField name="{name}" optype="continuous" dataType="\w+"\s*/>', txt)
    assert m is not None, name
    optype = "categorical" if categorical else "continuous"
    txt = (txt[:m.start()] + f'<DataField name="{name}" optype="{optype}" dataType="{data_type or dtype}">{children}'
           '</DataField>' + txt[m.end():])
    mf = [f'invalidValueTreatment="{invalid_treatment}"']
    if invalid_treatment in ("asMissing", "asValue"):  # the other two leave a missing value NaN
        mf.append(f'missingValueReplacement="{INT_MISSING_REPL if integer else MISSING_REPL}"')
    if invalid_treatment == "asValue":
        mf.append(f'invalidValueReplacement="{INT_INVALID_REPL if integer else INVALID_REPL}"')
    if attrs:
        mf.append(attrs)
    old = f'<MiningField name="{name}"/>'
    assert old in txt, name
    return txt.replace(old, f'<MiningField name="{name}" {" ".join(mf)}/>', 1)


def grid() -> List[Tuple[str, tuple, str, str, str]]:
    """(id, case, dtype, invalidValueTreatment, family) of every grid cell."""
    out = []
    for bname, b in BOUNDS.items():
        for fam, cases in families(b).items():
            for case in cases:
                for dtype in DTYPES:
                    for ivt in INVALID_TREATMENTS:
                        out.append((f"{case[0]}-{bname}-{dtype}-{ivt}", case, dtype, ivt, fam))
    for case in mask_cases():
        for ivt in INVALID_TREATMENTS:
            out.append((f"{case[0]}-{ivt}", case, "integer", ivt, "mask"))
    return out


def family_document(txt: str, family: str, dtype: str) -> Tuple[str, list]:
    """One document per treatment family: column j of a ``bench/synth.py`` document with enough
    fields takes cell j of the family (case x bound x invalidValueTreatment). Returns the document
    and its cells ``(case, invalidValueTreatment)``."""
    cells = []
    if family == "mask":
        cells = [(case, ivt) for case in mask_cases() for ivt in INVALID_TREATMENTS]
    else:
        for b in BOUNDS.values():
            cells += [(case, ivt) for case in families(b)[family] for ivt in INVALID_TREATMENTS]
    for j, (case, ivt) in enumerate(cells):
        txt = treat_field(txt, j, case[1], case[2], case[3], dtype, ivt)
    return txt, cells


def family_inputs(cells: list, n_features: int) -> np.ndarray:
    """fp32 rows that probe one column each (every probe value of that column's treatment in turn)
    while the other columns hold their safe values, then rows that probe two columns at once."""
    safe = np.zeros(n_features, dtype=F32)
    for j, (case, _) in enumerate(cells):
        safe[j] = case[5]
    rows = []
    for j, (case, _) in enumerate(cells):
        for v in probe_values(case[4]):
            r = safe.copy()
            r[j] = v
            rows.append(r)
    for j, (case, _) in enumerate(cells):
        k = (j + 5) % len(cells)
        for a, b in zip(probe_values(case[4]), probe_values(cells[k][0][4])[::-1]):
            r = safe.copy()
            r[j], r[k] = a, b
            rows.append(r)
    return np.array(rows, dtype=F32)


FAMILIES = [(fam, dt) for fam in ("interval-left", "interval-right", "outliers", "lists") for dt in DTYPES] + [
    ("integer", "integer"), ("mask", "integer")]
