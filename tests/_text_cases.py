"""Cases, a statement-by-statement twin and the oracles for the GPU CSV parser
(``ops/csrc/textparse.hip``: ``row_start_count``, ``row_start_scan``, ``row_start_write``,
``parse_rows``, ``parse_rows_lds``).

What the reader hands downstream is the kernel's matrix with every *flagged* row re-parsed on the
host (``DeviceTextReader._finish``), so comparing after that patch cannot tell a kernel that flags
everything, or writes garbage into rows it also flags, from a right one. Here the three things the
kernels themselves produce are pinned: the row starts, the raw matrix ``X_raw`` (NaN where a field
is missing, skipped, absent or not settled by the fast path) and the set of flagged rows.

* The **twin** restates the kernels over a ``bytes`` buffer (``twin_row_starts``,
  ``twin_fast_token``, ``twin_parse``, ``twin_dispatch``). ``twin_fast_token`` uses IEEE double
  arithmetic exactly as the kernel does: one correctly rounded multiply or divide by an exact power
  of ten, then double -> fp32. Every comparison is therefore exact: equal sets, equal fp32 bits.
* The **oracle** of the final matrix is ``native.RecordParser`` (``native/csrc/ingest.cpp``, the
  specification); for tokens the fast path accepts there is a second, independent one: correct
  rounding of the decimal to fp32 over ``fractions.Fraction``.
* ``device_parse`` calls the three entry points through ctypes exactly as
  ``DeviceTextReader._submit_copy`` / ``_submit_parse`` do and returns what the kernels wrote before
  any host patching, with guard elements behind every output.
* Every **case** is a small dict (``buf``, ``n_cols``, ``colmap``, ``F``, ``delim``, ``missing``,
  ``max_flagged``, ``misalign``) plus ``claims``: the byte placements and dispatch paths the case
  exists for, which ``test_text_cases.py`` asserts on the CPU.
* ``MUTANTS`` are named wrong restatements of the twin; each must change ``starts``, ``X_raw`` or
  the flag set of at least one case, or be proven unable to.

Not covered, on purpose: a delimiter that can occur inside a number (``.``, ``e``, ``-``, ``+``, a
digit) splits differently on host and device by construction (``docs/PARITY.md``); categorical
fields are not parsed on the device.
"""

import functools
import re
import struct
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

F32 = np.float32
TILE = 4096  # TP_TILE: bytes per row_start_* workgroup (16 per lane, 1024 per wave)
TP_TB = 256  # rows per parse_rows workgroup
PR_TB = 128  # rows per parse_rows_lds workgroup
PR_MAX_COLS = 256
MAX_MISSING = 8
MISSING_LEN = 16
GUARD = 64
SENTINEL32 = 0x5A5A5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A
DEFAULT_MISSING = ("NA", "NaN", "nan", "?", "null", "NULL")  # DeviceTextReader's default, "" dropped
SIX_COLMAP = (-1, 3, 0, -1, 2, 1)  # header junk, f3, f0, extra, f2, f1 of test_gpu_text.py
M64 = (1 << 64) - 1
P10 = [float(f"1e{k}") for k in range(24)]  # 1e0 .. 1e22 are exact doubles; 1e23 only for a mutant


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def same_matrix(a, b) -> bool:
    """Equal shapes, equal NaN masks, equal fp32 bits elsewhere (so -0.0 differs from 0.0)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and np.array_equal(bits(a)[~na], bits(b)[~nb]))


# --------------------------------------------------------------------------- the twin


def twin_row_starts(buf: bytes, mutant: Optional[str] = None) -> np.ndarray:
    """``is_row_start`` for every byte: a start follows ``'\\n'`` or is byte 0, and its line is not
    ``"\\n"`` or ``"\\r\\n"``."""
    b = np.frombuffer(buf, dtype=np.uint8)
    n = len(b)
    if n == 0:
        return np.zeros(0, np.int64)
    prev_nl = np.empty(n, bool)
    prev_nl[0] = mutant != "no-start-at-byte-0"
    prev_nl[1:] = b[:-1] == 10
    nxt_nl = np.zeros(n, bool)  # s + 1 < n && b[s + 1] == '\n'
    nxt_nl[:-1] = b[1:] == 10
    empty = b == 10
    if mutant != "crlf-line-not-empty":
        empty = empty | ((b == 13) & nxt_nl)
    return np.flatnonzero(prev_nl & ~empty).astype(np.int64)


def _f64_bits(d: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def twin_fast_token(tok: bytes, mutant: Optional[str] = None) -> Optional[np.float32]:
    """``fast_token`` over the trimmed token: the fp32 value, or ``None`` where the kernel flags."""
    s, e = 0, len(tok)
    neg = False
    if s < e and tok[s] in b"-+":
        neg = tok[s] == 0x2D
        s += 1
    w, digits, exp10, any_ = 0, 0, 0, False
    while s < e and 48 <= tok[s] <= 57:
        if w != 0 or tok[s] != 48 or mutant == "digits-count-leading-zeros":
            digits += 1
        w = (w * 10 + (tok[s] - 48)) & M64  # unsigned long long wraps
        s += 1
        any_ = True
    if s < e and tok[s] == 0x2E:
        s += 1
        while s < e and 48 <= tok[s] <= 57:
            if w != 0 or tok[s] != 48 or mutant == "digits-count-leading-zeros":
                digits += 1
            w = (w * 10 + (tok[s] - 48)) & M64
            exp10 -= 1
            s += 1
            any_ = True
    if not any_ or digits > (20 if mutant == "digits-limit-20" else 19):
        return None
    if s < e and tok[s] in b"eE":
        s += 1
        eneg = False
        if s < e and tok[s] in b"-+":
            eneg = tok[s] == 0x2D
            s += 1
        ev, ed = 0, 0
        while s < e and 48 <= tok[s] <= 57 and ed < (7 if mutant == "exponent-7-digits" else 6):
            ev = ev * 10 + (tok[s] - 48)
            s += 1
            ed += 1
        if ed == 0:
            return None
        exp10 += -ev if eneg else ev
    if s != e:
        return None
    # finish_decimal
    lim = 23 if mutant == "exp10-limit-23" else 22
    too_wide = w >= (1 << 53) if mutant == "w-ge-2^53" else w > (1 << 53)
    if too_wide or exp10 < -lim or exp10 > lim:
        return None
    d = float(w)  # exact: w <= 2^53
    d = d / P10[-exp10] if exp10 < 0 else d * P10[exp10]
    b = _f64_bits(d)
    be = (b >> 52) & 0x7FF
    if be != 0 and be >= 1023 - 126:
        if (b & ((1 << 29) - 1)) == (1 << 28) and mutant != "no-midpoint-test":
            return None
    elif d != 0.0:
        return None
    with np.errstate(over="ignore"):
        f = F32(d)
    return F32(-f) if neg else f


def _is_space(c: int) -> bool:
    return c == 0x20 or c == 0x09 or c == 0x22


def twin_trim(buf: bytes, s: int, e: int, mutant: Optional[str] = None) -> Tuple[int, int]:
    while s < e and (_is_space(buf[s]) or (mutant == "cr-trimmed-at-front" and buf[s] == 13)):
        s += 1
    while e > s and (_is_space(buf[e - 1]) or buf[e - 1] == 13):
        e -= 1
    return s, e


def missing_table(missing: Sequence[str]) -> bytes:
    """The device table: one NUL-padded ``MISSING_LEN`` slot per token (at least ``MAX_MISSING``)."""
    tab = bytearray(max(MAX_MISSING, len(missing)) * MISSING_LEN)
    for i, t in enumerate(missing):
        b = t.encode()
        assert 0 < len(b) < MISSING_LEN
        tab[i * MISSING_LEN: i * MISSING_LEN + len(b)] = b
    return bytes(tab)


def _twin_is_missing(tok: bytes, n_missing: int, table: bytes, mutant: Optional[str]) -> bool:
    miss = len(tok) == 0
    m = 0
    while not miss and m < n_missing:
        t = table[m * MISSING_LEN: (m + 1) * MISSING_LEN]
        k = 0
        while k < MISSING_LEN and t[k] and k < len(tok) and tok[k] == t[k]:
            k += 1
        miss = (k == MISSING_LEN or not t[k]) and (k == len(tok) or mutant == "missing-matched-as-prefix")
        m += 1
    return miss


def _twin_record(line: bytes, n_cols: int, colmap, F: int, delim: int, n_missing: int, table: bytes,
                 mutant: Optional[str]):
    """``parse_record`` over one line (without its ``'\\n'``): (row values, needs the host parser)."""
    out = [None] * F
    le = len(line)
    p, bad, c = 0, False, 0
    while c < n_cols and p <= le:
        te = p
        while te < le and line[te] != delim:
            te += 1
        oc = colmap[c]
        if oc >= 0:
            s, e = twin_trim(line, p, te, mutant)
            tok = line[s:e]
            if not _twin_is_missing(tok, n_missing, table, mutant):
                v = twin_fast_token(tok, mutant)
                if v is not None:
                    out[oc] = v
                else:
                    bad = True
        if te >= le and mutant != "no-ragged-break":
            break
        p = te + 1
        c += 1
    return out, bad


def twin_parse(buf: bytes, starts, n_cols: int, colmap, F: int, delim: bytes, missing: Sequence[str],
               mutant: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``(X_raw, flagged_rows)``: the matrix the parse kernels write themselves and the sorted rows
    with at least one token the fast path does not settle."""
    table = missing_table(missing)
    n_missing = len(missing)
    colmap = [int(c) for c in colmap]
    X = np.full((len(starts), F), np.nan, dtype=F32)
    flagged = []
    memo: Dict[bytes, tuple] = {}
    for r, st in enumerate(np.asarray(starts).tolist()):
        le = buf.find(b"\n", st)
        if le < 0:
            le = len(buf)
        line = buf[st:le]
        got = memo.get(line)
        if got is None:
            vals, bad = _twin_record(line, n_cols, colmap, F, delim[0], n_missing, table, mutant)
            cols = [j for j, v in enumerate(vals) if v is not None]
            got = memo[line] = (cols, np.array([vals[j] for j in cols], F32), bad)
        cols, vals, bad = got
        if cols:
            X[r, cols] = vals
        if bad:
            flagged.append(r)
    return X, np.array(flagged, dtype=np.int64)


def twin_lds(n_bytes: int, n_rows: int, F: int) -> Tuple[bool, int, int]:
    """The LDS arithmetic of ``pmml_text_parse``: (output tile + minimum text fit, ``cap`` as passed
    to ``parse_rows_lds``, dynamic LDS bytes)."""
    avg = n_bytes // n_rows + 1
    out_bytes = PR_TB * (F + 1) * 4
    cap = ((avg * PR_TB * 5 // 4 + 256) + 15) & ~15
    cap = max(cap, 4096)
    lds_max = 160 * 1024 - 2048
    fits = out_bytes + 4096 + 16 <= lds_max
    cap = min(cap, lds_max - out_bytes - 16)
    return fits, cap, out_bytes + cap + 16


def twin_dispatch(n_bytes: int, n_rows: int, n_cols: int, F: int, buf_aligned: bool, starts) -> List[str]:
    """The path of every workgroup of the parse launch: ``"global-kernel"`` (``parse_rows``, 256
    rows each), ``"lds"`` or ``"lds-fallback"`` (``parse_rows_lds``, 128 rows each; the fallback
    where the workgroup's byte span exceeds ``cap``)."""
    if n_rows <= 0:
        return []
    fits, cap, _ = twin_lds(n_bytes, n_rows, F)
    if not (n_cols <= PR_MAX_COLS and buf_aligned and fits):
        return ["global-kernel"] * (-(-n_rows // TP_TB))
    out = []
    for r0 in range(0, n_rows, PR_TB):
        nr = min(PR_TB, n_rows - r0)
        s_hi = int(starts[r0 + nr]) if r0 + nr < n_rows else n_bytes
        span = s_hi - (int(starts[r0]) & ~15)
        out.append("lds-fallback" if span > cap else "lds")
    return out


# --------------------------------------------------------------------------- named mutants

MUTANTS = ("no-midpoint-test", "w-ge-2^53", "digits-count-leading-zeros", "digits-limit-20", "exp10-limit-23",
           "exponent-7-digits",
           "cr-trimmed-at-front", "missing-matched-as-prefix", "crlf-line-not-empty", "no-start-at-byte-0",
           "no-ragged-break")
# "no-ragged-break" cannot show. The break leaves the column loop when a token ends at the line
# end (te >= le). Without it the next statement sets p = te + 1 = le + 1, and the loop's own guard
# `p <= le` ends the loop before another column is read. test_text_cases.py demonstrates that it
# changes nothing on any case.
INERT_MUTANTS = ("no-ragged-break",)


def twin_case(case: dict, mutant: Optional[str] = None):
    """(starts, X_raw, flagged rows) of a case under the twin or one of its mutants."""
    assert mutant is None or mutant in MUTANTS
    starts = twin_row_starts(case["buf"], mutant)
    X, flagged = twin_parse(case["buf"], starts, case["n_cols"], case["colmap"], case["F"], case["delim"],
                            case["missing"], mutant)
    return starts, X, flagged


def _mutant(name):
    def run(case):
        return twin_case(case, name)

    run.__name__ = "mutant_" + re.sub(r"\W", "_", name)
    return run


mutant_no_midpoint_test = _mutant("no-midpoint-test")
mutant_w_ge_2_53 = _mutant("w-ge-2^53")
mutant_digits_count_leading_zeros = _mutant("digits-count-leading-zeros")
mutant_digits_limit_20 = _mutant("digits-limit-20")  # 2^64 + 1 wraps to w = 1 and would read as 1.0
mutant_exp10_limit_23 = _mutant("exp10-limit-23")
mutant_exponent_7_digits = _mutant("exponent-7-digits")
mutant_cr_trimmed_at_front = _mutant("cr-trimmed-at-front")
mutant_missing_matched_as_prefix = _mutant("missing-matched-as-prefix")
mutant_crlf_line_not_empty = _mutant("crlf-line-not-empty")
mutant_no_start_at_byte_0 = _mutant("no-start-at-byte-0")
mutant_no_ragged_break = _mutant("no-ragged-break")
MUTANT_FUNCS = {name: globals()["mutant_" + re.sub(r"\W", "_", name)] for name in MUTANTS}


# --------------------------------------------------------------------------- oracles


class _Schema:
    values: dict = {}

    def is_string(self, field) -> bool:
        return False


class Fields:
    """What ``RecordParser`` and ``DeviceTextReader`` need of a compiled model: F numeric fields."""

    def __init__(self, F: int):
        self.active_fields = [f"f{j}" for j in range(F)]
        self.schema = _Schema()


def columns_of(colmap) -> List[str]:
    """A header that yields ``colmap``: ``f<j>`` for output column j (twice where two input columns
    share one), a name no field has for a skipped column."""
    return [f"f{oc}" if oc >= 0 else f"skip{c}" for c, oc in enumerate(colmap)]


def host_parser(case: dict):
    from flink_jpmml_amd import native

    return native.RecordParser(Fields(case["F"]), columns_of(case["colmap"]), delimiter=case["delim"].decode(),
                               missing=[""] + list(case["missing"]))


def host_parse(case: dict) -> np.ndarray:
    """The final matrix: ``native.RecordParser`` over the whole buffer."""
    m, used = host_parser(case).parse(case["buf"])
    assert used == len(case["buf"])
    return np.array(m, dtype=F32)


_DECIMAL = re.compile(rb"^([+-]?)(\d*)(?:\.(\d*))?(?:[eE]([+-]?\d+))?$")


def decimal_fraction(tok: bytes) -> Tuple[Fraction, bool]:
    """The exact value of a plain decimal token and whether it carries a minus sign."""
    m = _DECIMAL.match(tok)
    assert m and (m.group(2) or m.group(3)), tok
    frac = m.group(3) or b""
    x = Fraction(int((m.group(2) or b"") + frac or b"0")) * Fraction(10) ** (int(m.group(4) or 0) - len(frac))
    return x, m.group(1) == b"-"


def f32_correctly_rounded(tok: bytes) -> np.float32:
    """The fp32 nearest to the decimal token, ties to even, over rationals (the approach of
    ``test_native_ingest._f32_correctly_rounded``)."""
    x, neg = decimal_fraction(tok)
    if x == 0:
        return F32(-0.0 if neg else 0.0)
    c = F32(float(x))  # within one ulp: the double step can round twice
    cands = [np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))]
    cands = [f for f in cands if np.isfinite(f)]
    best = min(cands, key=lambda f: (abs(Fraction(float(f)) - x), int(bits(f)) & 1))
    return F32(-best if neg else best)


# --------------------------------------------------------------------------- direct harness


def device_parse(lib, device, buf: bytes, n_cols: int, colmap, F: int, delim: bytes, missing: Sequence[str],
                 max_flagged: int, misalign: int = 0) -> dict:
    """``pmml_text_rows_count`` -> ``pmml_text_rows_write`` -> ``pmml_text_parse`` as
    ``DeviceTextReader._submit_copy`` / ``_submit_parse`` call them, nothing patched afterwards.

    ``starts``, ``X``, the tile counts and the flag list (with its counter in the slot right after
    the list, as in the reader) are followed by ``GUARD`` sentinel elements each; the unused part of
    the flag list holds the sentinel too. Returns the used parts, the guards and the return codes."""
    import ctypes

    import torch

    from flink_jpmml_amd.ops._lib import TextParseArgs

    n = len(buf)
    assert n > 0 and buf[-1:] == b"\n"
    base = torch.empty(n + misalign, dtype=torch.uint8, device=device)
    dev = base[misalign:]
    dev.copy_(torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()))
    assert dev.data_ptr() % 16 == misalign % 16
    stream = torch.cuda.current_stream(device).cuda_stream
    tiles = -(-n // TILE)
    counts = torch.full((tiles + 1 + GUARD,), SENTINEL32, dtype=torch.int32, device=device)
    rc_count = lib.pmml_text_rows_count(stream, dev.data_ptr(), n, counts.data_ptr())
    assert rc_count == 0, rc_count
    rows = int(counts[tiles].item())
    assert 0 <= rows <= n
    starts = torch.full((max(1, rows) + GUARD,), SENTINEL64, dtype=torch.int64, device=device)
    X = torch.full((rows * F + GUARD,), SENTINEL32, dtype=torch.int32, device=device)
    flags = torch.full((max_flagged + 1 + GUARD,), SENTINEL32, dtype=torch.int32, device=device)
    flags[max_flagged: max_flagged + 1].zero_()
    rc_write = lib.pmml_text_rows_write(stream, dev.data_ptr(), n, counts.data_ptr(), starts.data_ptr())
    assert rc_write == 0, rc_write
    colmap_dev = torch.tensor(list(colmap), dtype=torch.int32, device=device)
    table = torch.from_numpy(np.frombuffer(missing_table(missing), dtype=np.uint8).copy()).to(device)
    a = TextParseArgs()
    a.buf, a.n_bytes, a.starts, a.n_rows = dev.data_ptr(), n, starts.data_ptr(), rows
    a.n_cols, a.colmap, a.F = n_cols, colmap_dev.data_ptr(), F
    a.delim = delim
    a.n_missing, a.missing = len(missing), table.data_ptr()
    a.X = X.data_ptr()
    a.flagged, a.max_flagged = flags.data_ptr(), max_flagged
    a.n_flagged = flags[max_flagged:].data_ptr()
    rc = lib.pmml_text_parse(stream, ctypes.byref(a))
    torch.cuda.synchronize(device)
    counts_h, starts_h, X_h, flags_h = (t.cpu().numpy() for t in (counts, starts, X, flags))
    return {
        "rc": rc,
        "rows": rows,
        "tile_offsets": counts_h[:tiles],
        "starts": starts_h[:rows],
        "X_raw": X_h[: rows * F].view(F32).reshape(rows, F),
        "n_flagged": int(flags_h[max_flagged]),
        "flag_list": flags_h[:max_flagged],
        "guards": {"counts": counts_h[tiles + 1:], "starts": starts_h[max(1, rows):], "X": X_h[rows * F:],
                   "flags": flags_h[max_flagged + 1:]},
    }


# --------------------------------------------------------------------------- buffers


class Lines:
    """A buffer built line by line. ``row()`` appends a record whose single payload is the running
    row number (so a row's value identifies it), padded with blanks to an exact length."""

    def __init__(self):
        self.parts: List[bytes] = []
        self.n = 0
        self.rows = 0
        self.values: List[float] = []

    def raw(self, b: bytes) -> None:
        self.parts.append(b)
        self.n += len(b)

    def row(self, length: Optional[int] = None, lead: int = 0, payload: Optional[bytes] = None) -> int:
        """Returns the byte the row starts at."""
        self.rows += 1
        pay = payload if payload is not None else str(self.rows).encode()
        length = len(pay) + 1 if length is None else length
        pad = length - 1 - len(pay)
        assert pad >= 0, (length, pay)
        lead = min(lead, pad)
        at = self.n
        self.raw(b" " * lead + pay + b" " * (pad - lead) + b"\n")
        self.values.append(float(pay))
        return at

    def fill_to(self, target: int, rng) -> None:
        """Rows of random lengths (and now and then an empty line) up to exactly ``target`` bytes."""
        assert target == self.n or target - self.n >= 9, (self.n, target)
        while target - self.n > 40:
            k = int(rng.integers(0, 12))
            if k == 0:
                self.raw(b"\n")
            elif k == 1:
                self.raw(b"\r\n")
            else:
                self.row(len(str(self.rows + 1)) + 1 + int(rng.integers(0, 12)), lead=int(rng.integers(0, 4)))
        if target > self.n:
            self.row(target - self.n, lead=int(rng.integers(0, 4)))
        assert self.n == target

    def bytes(self) -> bytes:
        return b"".join(self.parts)


def _case(name: str, buf: bytes, n_cols: int = 1, colmap=(0,), F: int = 1, delim: bytes = b",",
          missing: Sequence[str] = DEFAULT_MISSING, max_flagged: int = 1 << 16, misalign: int = 0, **claims) -> dict:
    assert buf.endswith(b"\n") and len(delim) == 1 and len(colmap) == n_cols
    return {"name": name, "buf": buf, "n_cols": n_cols, "colmap": tuple(colmap), "F": F, "delim": delim,
            "missing": tuple(missing), "max_flagged": max_flagged, "misalign": misalign, "claims": claims}


START_PLACEMENTS = (0, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)
CRLF_PLACEMENTS = (15, 1023, 4095)  # the '\r' of an empty "\r\n" line; its '\n' is the edge byte


def _placed(name: str, at: int, seed: int, crlf: bool = False) -> dict:
    rng = np.random.default_rng(seed)
    L = Lines()
    if crlf:
        L.fill_to(at, rng)
        L.raw(b"\r\n")
        want = L.row()  # the record right after the empty line
    else:
        L.fill_to(at, rng)
        want = L.row()
    L.fill_to(2 * TILE + 200 + int(rng.integers(0, 64)), rng)
    last = L.row(payload=b"7")  # the last record starts at n - 2
    c = _case(name, L.bytes(), start_at=[want, last], values=list(L.values))
    if crlf:
        c["claims"]["crlf_at"] = at
    return c


def _dense_long_mix(n_tiles: int, seed: int) -> Lines:
    """Exactly ``n_tiles`` tiles: stretches of ``"1\\n"`` lines (2048 starts per tile, 8 per lane),
    stretches of 5000-byte lines (tiles without a start) and short numbered lines."""
    rng = np.random.default_rng(seed)
    L = Lines()
    total = n_tiles * TILE - int(rng.integers(1, TILE - 1))  # a partial last tile
    dense = b"1\n" * (TILE // 2)
    while total - L.n > 12 * TILE:
        k = int(rng.integers(0, 8))
        if k == 0:  # one or two dense tiles, starting anywhere
            t = int(rng.integers(1, 3))
            L.raw(dense * t)
            L.rows += t * (TILE // 2)
            L.values.extend([1.0] * (t * (TILE // 2)))
        elif k == 1:
            for _ in range(int(rng.integers(1, 30))):
                L.row(len(str(L.rows + 1)) + 1 + int(rng.integers(0, 30)))
        else:
            for _ in range(int(rng.integers(1, 12))):
                L.row(5000, lead=int(rng.integers(0, 4000)))
    L.fill_to(total - 2, rng)
    L.row(payload=b"7")
    assert -(-L.n // TILE) == n_tiles
    return L


@functools.lru_cache(maxsize=None)
def row_cases() -> List[dict]:
    """One column, F = 1: what is under test is where rows start."""
    cases = [_placed(f"start@{at}", at, 100 + i) for i, at in enumerate(START_PLACEMENTS)]
    cases += [_placed(f"crlf@{at}", at, 200 + i, crlf=True) for i, at in enumerate(CRLF_PLACEMENTS)]

    rng = np.random.default_rng(300)
    L = Lines()
    L.fill_to(TILE - 30, rng)
    lo = L.n
    for i in range(40):
        L.raw(b"\r\n" if rng.random() < 0.5 else b"\n")
    hi = L.n
    after = L.row()
    L.fill_to(TILE + 600, rng)
    cases.append(_case("empty-run@4096", L.bytes(), empty_run=(lo, hi), start_at=[after], values=list(L.values)))

    cases.append(_case("only-empty-lines", b"\n\r\n\n\n\r\n\r\n\n" * 700, values=[]))
    cases.append(_case("newline", b"\n", values=[]))
    cases.append(_case("seven", b"7\n", start_at=[0], values=[7.0]))
    n = 3 * TILE // 2
    cases.append(_case("dense-3-tiles", b"1\n" * n, values=[1.0] * n, per_tile=TILE // 2))

    rng = np.random.default_rng(301)
    L = Lines()
    L.row(9000, lead=4000)
    L.fill_to(9000 + 700, rng)
    cases.append(_case("long-line-then-short", L.bytes(), start_at=[0, 9000], values=list(L.values),
                       empty_tiles=[1]))

    for tiles, seed in ((1025, 302), (2051, 303)):
        L = _dense_long_mix(tiles, seed)
        cases.append(_case(f"tiles-{tiles}", L.bytes(), values=list(L.values), n_tiles=tiles))
    return cases


def generated_tokens() -> List[bytes]:
    """The random generators of ``test_gpu_text._tokens`` (rounding corpus, random plain decimals up
    to 21 digits with exponents, exact fp32 midpoints, its fixed oddities)."""
    from tests.test_gpu_text import _tokens

    return [t.encode() for t in _tokens(np.random.default_rng(20408))]


def placed_tokens() -> List[bytes]:
    t: List[bytes] = []
    d19, d20 = b"1234567890123456789", b"12345678901234567890"
    t += [d19, d20, b"0" * 25 + d19, b"0" * 25 + d20, b"0.000" + d19, b"0.000" + d20, b"9" * 19, b"9" * 20,
          d19[:10] + b"." + d19[10:], d20[:10] + b"." + d20[10:], b"18446744073709551615", b"18446744073709551616",
          b"18446744073709551617", b"18446744073709551617e-3", b"0" * 25 + b"9007199254740992",
          b"00009007199254740992", b"0.000" + b"9007199254740992", b"90071992547409920000", b"9007199254740992000", b"00000000000000000001", b"0.0000000000000000000", b"0" * 30]
    for w in (2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2):
        s = str(w).encode()
        t += [s, b"-" + s, s[:8] + b"." + s[8:], s[:1] + b"." + s[1:], b"0." + s, s + b"e5", s + b"e-20", s + b"e22",
              s + b"e23"]
    t += [b"1e22", b"1e23", b"1e-22", b"1e-23", b"123.456e20", b"123.456e25", b"123.456e26", b"0." + b"0" * 21 + b"1",
          b"0." + b"0" * 22 + b"1", b"1e000001", b"1e0000001", b"1e000022", b"1e+000022", b"1E-000022", b"1e999999",
          b"1e-999999"]
    t += [b"1e", b"1e+", b"1e-", b"e5", b".", b"+.", b"-.5", b"5.", b"+", b"-", b"--1", b"+-1", b"+5", b".e5", b"5.e1",
          b"1e5.", b"1e5e5", b"1.5.2"]
    t += [b"-0", b"-0.0", b"0e99999", b"0e22", b"0e23", b"-0e5", b"+0", b"0", b"0.0e-999"]
    for k in range(2 ** 23, 2 ** 23 + 300):  # half-integer fp32 midpoints and their decimal neighbours
        t += [b"%d.5" % k, b"%d.4" % k, b"%d.6" % k]
    for k in range(2 ** 24 + 1, 2 ** 24 + 100, 2):  # odd integers above 2^24 are midpoints too
        t += [b"%d" % k, b"%d" % (k - 1), b"%d" % (k + 1)]
    t += [b"inf", b"Infinity", b"INF", b"-inf", b"+inf", b"nan(abc)", b"3.5e38", b"3.4028235e38", b"1e-46", b"1e-45",
          b"1e400", b"1_0", b"0x10", b"1.17549435e-38", b"1.1754942e-38"]
    t += [b"1\x805", b"\xc3\xa95", b"1\x005", b"\x00", b"5\x00"]
    t += [b" 2.5 ", b'"3.25"', b"\t-1\t", b"5\r", b"\r5", b" \r 5 \r", b'" 4 "', b"  ", b'""', b"5 \r\t\"", b" N A ",
          b" NA ", b"\rNA"]
    assert not any(b"," in x or b"\n" in x for x in t)
    return t


def _token_buf(tokens: Sequence[bytes]) -> bytes:
    """One token per record in column 0, a constant 0 in column 1: no line is empty and the flag
    set maps one to one onto the tokens."""
    return b"".join(tok + b",0\n" for tok in tokens)


@functools.lru_cache(maxsize=None)
def token_cases() -> List[dict]:
    out = []
    for name, toks in (("tokens-generated", generated_tokens()), ("tokens-placed", placed_tokens())):
        out.append(_case(name, _token_buf(toks), n_cols=2, colmap=(0, 1), F=2, tokens=list(toks)))
    return out


MISSING8 = ("NA", "NaN", "nan", "?", "null", "NULL", "-999", "missing_value_x")


@functools.lru_cache(maxsize=None)
def missing_cases() -> List[dict]:
    assert len(MISSING8) == MAX_MISSING and max(len(m) for m in MISSING8) == MISSING_LEN - 1
    toks = [m.encode() for m in MISSING8]
    toks += [b" NA ", b'"null"', b"-999\r", b" missing_value_x\t"]  # trimmed, then matched
    toks += [b"N", b"Na", b"nul", b"-99", b"-", b"missing_value_", b"m"]  # strict prefixes of a missing token
    toks += [b"NAN", b"NA.", b"nullx", b"-9990", b"-999.0", b"??", b"missing_value_xy", b"missing_value_x12"]
    toks += [b"na", b"Null", b"nAn", b"MISSING_VALUE_X", b"null\x00", b"N\x00A"]  # letter case, NUL
    toks += [b"1.5", b"-2", b"", b"abc", b"999", b"-999e0"]
    buf = _token_buf(toks)
    return [
        _case("missing-8-tokens", buf, n_cols=2, colmap=(0, 1), F=2, missing=MISSING8, tokens=list(toks)),
        _case("missing-default", buf, n_cols=2, colmap=(0, 1), F=2, tokens=list(toks)),
        _case("missing-empty-table", buf, n_cols=2, colmap=(0, 1), F=2, missing=(), tokens=list(toks)),
    ]


DELIMS = (b",", b";", b"\t", b"|", b" ")


def _shape_lines(d: bytes, rng) -> List[bytes]:
    """Six-column line shapes under delimiter ``d`` (tokens hold no delimiter, so blanks and tabs
    inside tokens appear only where they are not the delimiter)."""
    pool = [b"1.5", b"-2", b"", b"NA", b"abc", b"3e2", b"0.25", b"16777217", b"-0", b"7", b"1e-40", b"+4", b"?"]
    if d not in b" ":
        pool += [b" 2.5 ", b"  "]
    if d != b"\t":
        pool += [b"\t-1\t"]
    pool += [b'"3.25"', b"5\r"]

    def row(n):
        return [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]

    lines = []
    for n in (6, 6, 6, 1, 2, 3, 4, 5, 7, 8, 9):  # full, ragged, extra columns
        lines.append(d.join(row(n)))
    lines.append(d.join(row(6)) + d)  # a trailing delimiter
    lines.append(d.join(row(3)) + d)  # ragged with a trailing delimiter
    lines.append(b"   ")  # blanks only
    lines.append(d * 5)  # delimiters only
    lines.append(d * 9)
    lines.append(d.join(row(6)) + b"\r")  # CRLF line end
    lines.append(b"")  # an empty line: no record
    lines.append(b"\r")
    lines.append(d.join([b"9"] * 6))
    for _ in range(140):  # more than one workgroup
        lines.append(d.join(row(int(rng.integers(1, 9)))))
    return lines


@functools.lru_cache(maxsize=None)
def shape_cases() -> List[dict]:
    out = []
    for i, d in enumerate(DELIMS):
        rng = np.random.default_rng(400 + i)
        buf = b"\n".join(_shape_lines(d, rng)) + b"\n"
        tag = {b",": "comma", b";": "semicolon", b"\t": "tab", b"|": "bar", b" ": "blank"}[d]
        out.append(_case(f"shapes-{tag}", buf, n_cols=6, colmap=SIX_COLMAP, F=4, delim=d))
        out.append(_case(f"shapes-{tag}-one-column-kept", buf, n_cols=6, colmap=(-1, -1, -1, -1, 0, -1), F=1, delim=d))
        # input columns 1 and 4 both feed output column 1: the later one wins when it is present
        dup = [b"1" + d + b"2" + d + b"3" + d + b"4" + d + b"5" + d + b"6",  # later present
               b"1" + d + b"2" + d + b"3" + d + b"4" + d + d + b"6",  # later empty: the earlier value stays
               b"1" + d + b"2" + d + b"3" + d + b"4" + d + b"NA" + d + b"6",  # later a missing token
               b"1" + d + b"2" + d + b"3" + d + b"4" + d + b"junk" + d + b"6",  # later unsettled: flagged, earlier stays
               b"1" + d + b"2" + d + b"3",  # later absent
               b"1" + d + d + b"3" + d + b"4" + d + b"5" + d + b"6",  # earlier empty
               b"1" + d + b"junk" + d + b"3" + d + b"4" + d + b"5" + d + b"6"]  # earlier unsettled, later written
        out.append(_case(f"shapes-{tag}-two-columns-one-field", b"\n".join(dup) + b"\n", n_cols=6,
                         colmap=(0, 1, 2, -1, 1, 3), F=4, delim=d))
    return out


def _digit_rows(n_rows: int, n_fields, seed: int) -> bytes:
    """Rows of one-digit fields (2 bytes each with the delimiter); ``n_fields(r)`` fields in row r.
    The digit depends on row and column, so a swapped row or column shows."""
    rng = np.random.default_rng(seed)
    salt = rng.integers(0, 10, 1024)
    lines = []
    for r in range(n_rows):
        k = n_fields(r)
        lines.append(b",".join(b"%d" % ((int(salt[(r * 7 + c) % 1024]) + r + 3 * c) % 10) for c in range(k)))
    return b"\n".join(lines) + b"\n"


def _six_column_rows(n_rows: int, seed: int, junk_row: Optional[int] = None) -> bytes:
    rng = np.random.default_rng(seed)
    lines = []
    for r in range(n_rows):
        row = [b"%.4g" % v for v in rng.standard_normal(6)]
        if r % 37 == 5:
            row[2] = b"16777217"  # a midpoint: flagged
        if r == junk_row:
            row[3] = b"x" * 65536  # a skipped column
        lines.append(b",".join(row))
    return b"\n".join(lines) + b"\n"


@functools.lru_cache(maxsize=None)
def dispatch_cases() -> List[dict]:
    out = []
    rev = tuple(range(199, -1, -1))
    out.append(_case("lds-F200", _digit_rows(300, lambda r: 200, 500), n_cols=200, colmap=rev, F=200,
                     paths={"lds"}, lds_over_64k=True))
    out.append(_case("lds-F256-ragged", _digit_rows(300, lambda r: 3 if r % 7 else 256, 501), n_cols=256, colmap=tuple(range(256)),
                     F=256, paths={"lds"}, lds_over_64k=True))
    cm = [-1] * 257
    cm[256] = 0
    out.append(_case("global-257-columns", _digit_rows(300, lambda r: 257 if r % 3 else 200, 502), n_cols=257,
                     colmap=tuple(cm), F=1, paths={"global-kernel"}))
    out.append(_case("global-F307", _digit_rows(300, lambda r: 307 if r % 5 else 11, 503), n_cols=307,
                     colmap=tuple(range(307)), F=307, paths={"global-kernel"}))
    out.append(_case("global-misaligned", _six_column_rows(300, 504), n_cols=6, colmap=SIX_COLMAP, F=4, misalign=1,
                     paths={"global-kernel"}))
    out.append(_case("lds-fallback-long-field", _six_column_rows(300, 505, junk_row=5), n_cols=6, colmap=SIX_COLMAP,
                     F=4, paths={"lds", "lds-fallback"}, groups=["lds-fallback", "lds", "lds"]))
    for n in (129, 257):
        out.append(_case(f"rows-{n}", _six_column_rows(n, 506 + n), n_cols=6, colmap=SIX_COLMAP, F=4, paths={"lds"},
                         n_rows=n))
    return out


CAPACITY_ROWS = (3, 130, 131, 260, 299)
CAPACITIES = (0, 4, 5, 6, 64)


def capacity_buffer() -> bytes:
    """300 six-column records (three LDS workgroups), exactly five of which are flagged."""
    rng = np.random.default_rng(600)
    lines = []
    for r in range(300):
        row = [b"%d.25" % int(v) for v in rng.integers(-1000, 1000, 6)]
        if r in CAPACITY_ROWS:
            row[1 + r % 2] = b"16777217"  # a mapped column
        lines.append(b",".join(row))
    return b"\n".join(lines) + b"\n"


@functools.lru_cache(maxsize=None)
def capacity_cases() -> List[dict]:
    buf = capacity_buffer()
    return [_case(f"capacity-{m}", buf, n_cols=6, colmap=SIX_COLMAP, F=4, max_flagged=m,
                  flagged_rows=list(CAPACITY_ROWS)) for m in CAPACITIES]


def all_cases() -> List[dict]:
    return row_cases() + token_cases() + missing_cases() + shape_cases() + dispatch_cases() + capacity_cases()


def case_named(name: str) -> dict:
    return {c["name"]: c for c in all_cases()}[name]


@functools.lru_cache(maxsize=None)
def twin_of(name: str):
    """The twin's (starts, X_raw, flagged rows) of a case, computed once."""
    return twin_case(case_named(name))


# --------------------------------------------------------------------------- reader-level corpora


def messy_corpus(seed: int = 7, n_lines: int = 3000) -> bytes:
    """The messy corpus of ``test_gpu_text._write_csv`` without its header, plus ``"\\r\\n"`` empty
    lines: six columns, ragged and over-long rows, CRLF line ends. Ends with a newline."""
    rng = np.random.default_rng(seed)
    toks = [t for t in generated_tokens() + placed_tokens()[:200] if b"," not in t]
    lines = []
    for _ in range(n_lines):
        k = int(rng.integers(0, 10))
        if k == 0:
            lines.append(b"")
            continue
        if k == 9:
            lines.append(b"\r")
            continue
        row = [toks[int(rng.integers(0, len(toks)))] for _ in range(6)]
        if k == 1:
            row = row[: int(rng.integers(1, 6))]
        elif k == 2:
            row += [b"9", b"9"]
        lines.append(b",".join(row) + (b"\r" if k == 3 else b""))
    return b"\n".join(lines) + b"\n"
