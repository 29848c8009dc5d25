"""Cases, reference, checker and mutants of the row-grouping kernels (``ops/csrc/grouped.hip``).

The three entry points only move bits and add integers, so everything is held exactly:

* ``ref_group_rows`` / ``ref_ungroup`` / ``ref_group_slice`` are plain sequential numpy restatements
  of the contracts in the comments of ``grouped.hip`` (rows placed in arrival order);
* the slot of a row inside its group depends on atomic timing on the device, so the checkers
  (``check_group_rows`` / ``check_ungroup`` / ``check_group_slice``) assert invariants — ranges,
  bijections, bit-equal rows, exact tables, untouched guards — never equality with the reference's
  permutation;
* ``MUTANTS`` names one-line changes of the reference; ``tests/test_group_cases.py`` proves the
  checkers reject each of them, and ``tests/test_gpu_grouping.py`` runs the same grid (``GRID``)
  through the kernels.

A checker reads *buffers*: dicts of flat numpy arrays laid out as the GPU test lays out its torch
tensors — ``GUARD`` guard elements, an optional one-float offset (``x_off`` / ``xg_off``: the base
leaves its 16-byte boundary and the kernels must take the 4-byte copy path), the body, ``GUARD``
guard elements. ``emulate_*`` builds those buffers from the reference (or a mutant of it).

Row ``r`` of ``X`` carries ``float(r)`` in column 0, so a misplaced row is named in the failure; the
other cells hold small integers or a special value (``tests/_boundary.py::SPECIALS`` and NaNs with
payloads), the pad columns ``F..ldx`` a pattern of their own. No torch at module level."""

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from tests._boundary import SPECIALS

GROUP_TB = 256      # rows per group_rows / group_place workgroup
COUNT_ROWS = 4096   # rows per group_count workgroup
GROUP_MAXK = 1024
GUARD = 8           # guard elements before and behind every buffer (32 bytes of fp32 / int32)
GUARD32 = np.uint32(0xA5A5A5A5)  # as fp32 a finite negative number, as int32 negative: never a valid answer
GUARD8 = np.uint8(0xA5)
NAN32 = np.uint32(0x7FC00000)
PAD32 = np.uint32(0xBAD00000)    # | row: what the pad columns of X hold
CODE_DTYPES = {1: np.uint8, 2: np.int16, 4: np.int32}
TILES = (64, 128, 256)
SPECIAL_BITS = np.array([np.float32(v).view(np.uint32) for v, _ in SPECIALS] +
                        [0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE], dtype=np.uint32)  # + NaN payloads

MUTANTS = {
    "slot-off-by-one": "a row lands one slot behind its own",
    "shared-slot": "the first two rows of a group share a slot",
    "inclusive-prefix": "inclusive instead of exclusive prefix of the counts",
    "no-model-counted": "a tile_rows == 0 code counted into row_start",
    "tiles-floor": "floor instead of ceil for an entry's tiles",
    "tiles-code-order": "tile_start taken in code order instead of `order`",
    "codes-u16": "codes read as unsigned 16-bit",
    "pad-copied": "a row copied with its pad columns (ldx words instead of F)",
    "counts-not-cleared": "counts left as counted",
    "ticket-not-reset": "ticket left at the number of counting workgroups",
    "invalid-unanswered": "a row without a model left unanswered in out_s / out_v",
    "ungroup-no-gather": "ungroup reads sg[j] instead of sg[inv[j]]",
    "second-pair-skipped": "ungroup's second output pair not written",
}


# --------------------------------------------------------------------------- the grid


@dataclass(frozen=True)
class Spec:
    name: str
    n: int
    K: int
    code_bytes: int
    F: int = 4
    pad: int = 0            # ldx = F + pad
    x_off: int = 0          # floats the X base sits behind a 16-byte boundary
    xg_off: int = 0         # ... and the Xg base
    dist: str = "random"    # one | robin | random | absent | heavy | invalid | exact
    models: str = "all"     # all | half | none: which codes have tile_rows > 0
    inv_share: float = 0.125  # share of rows given an invalid code (where the width can express one)

    @property
    def ldx(self) -> int:
        return self.F + self.pad

    @property
    def vec4(self) -> bool:
        """Whether the kernels take the float4 copy path (pmml_group_rows / pmml_group_slice)."""
        return self.F % 4 == 0 and self.ldx % 4 == 0 and self.x_off == 0 and self.xg_off == 0


def _grid() -> List[Spec]:
    S = Spec
    g = [
        # row counts: the GROUP_TB = 256 and COUNT_ROWS = 4096 boundaries; 12289 = four counting workgroups
        S("n1", 1, 1, 1, F=1, dist="one", inv_share=0.0),
        S("n255", 255, 2, 1, F=3),
        S("n256", 256, 2, 2, F=4),
        S("n257", 257, 3, 4, F=5, pad=1),
        S("n4095", 4095, 7, 1, F=16),
        S("n4096", 4096, 7, 2, F=16, pad=4),
        S("n4097", 4097, 7, 4, F=4, pad=4),
        S("n12289", 12289, 13, 2, F=4, dist="heavy"),
        # model counts per code width
        S("k1-i32", 600, 1, 4, dist="one", inv_share=0.25),
        S("k2-i16", 600, 2, 2, dist="robin"),
        S("k200-u8", 700, 200, 1),                 # codes 200..255 are invalid
        S("k255-u8", 700, 255, 1, dist="robin"),
        S("k256-u8", 700, 256, 1),                 # no invalid code exists
        S("k256-i16", 700, 256, 2),
        S("k257-i16", 1300, 257, 2, dist="robin"),  # n_entries = 257: the scan gives threads two elements
        S("k1024-i16", 2500, 1024, 2, dist="robin"),  # n_entries = K = 1024
        S("k255-i32", 700, 255, 4, dist="heavy"),
        S("k257-i32", 1300, 257, 4, models="half"),
        S("k1024-i32", 4097, 1024, 4, models="half"),
        # code distributions
        S("d-one", 1000, 12, 1, dist="one", inv_share=0.0),
        S("d-robin", 1000, 12, 2, dist="robin", inv_share=0.0),
        S("d-absent-u8", 1000, 12, 1, dist="absent"),
        S("d-absent-i32", 1000, 12, 4, dist="absent", F=5, pad=1),
        S("d-heavy", 1000, 12, 4, dist="heavy"),
        S("d-invalid-u8", 1000, 12, 1, dist="invalid"),
        S("d-invalid-i16", 1000, 12, 2, dist="invalid", F=3, pad=1),
        S("d-invalid-i32", 1000, 12, 4, dist="invalid"),
        S("d-half-u8", 1000, 12, 1, models="half", F=3, pad=4),
        S("d-half-i16", 4097, 12, 2, models="half"),
        # tiles: counts of exactly tile_rows, tile_rows + 1 and 1; no entries at all
        S("t-exact-i16", 340, 4, 2, dist="exact"),
        S("t-exact-i32", 341, 4, 4, dist="exact", F=16, pad=4, x_off=1),
        S("t-none-u8", 600, 5, 1, models="none"),
        S("t-none-i32", 4097, 5, 4, models="none", F=5, pad=4),
        # back-to-back slices on the same tables (K = 13, as n12289)
        S("seq-b", 4097, 13, 2, F=4, dist="absent"),
        S("seq-invalid", 5000, 13, 2, F=4, dist="invalid"),
        S("seq-c", 257, 13, 2, F=4, dist="robin"),
    ]
    # layouts: every F x pitch, and the bases leaving their 16-byte boundary where VEC4 would apply
    for i, F in enumerate((1, 3, 4, 5, 16)):
        for j, pad in enumerate((0, 1, 4)):
            g.append(S(f"f{F}-p{pad}", 300 + 7 * j, 5, (1, 2, 4)[(i + j) % 3], F=F, pad=pad))
    g += [S("f4-p0-xoff", 300, 5, 1, F=4, x_off=1), S("f4-p4-goff", 300, 5, 2, F=4, pad=4, xg_off=1),
          S("f16-p0-goff", 300, 5, 4, F=16, xg_off=1), S("f16-p4-xoff", 300, 5, 1, F=16, pad=4, x_off=1)]
    return g


GRID: List[Spec] = _grid()
NAMES = [s.name for s in GRID]
SEQUENCE = ["n12289", "seq-b", "seq-invalid", "seq-c"]  # one set of tables, slice after slice
assert len(set(NAMES)) == len(NAMES)


def tables(K: int, models: str):
    """``(tile_rows[K], order)`` of a model set: a function of ``K`` and ``models`` alone, so cases
    with equal ``K`` and ``models`` can share the device tables. ``order`` lists the codes that have
    a model in launch order — never the identity when there are two or more."""
    tile_rows = np.array([TILES[k % 3] for k in range(K)], dtype=np.int32)
    if models == "half":
        tile_rows[1::2] = 0
    elif models == "none":
        tile_rows[:] = 0
    has = np.flatnonzero(tile_rows > 0)
    order = np.roll(has[::-1], len(has) // 3).astype(np.int32)
    assert len(has) < 2 or not np.array_equal(order, has)
    return tile_rows, order


def _invalid_codes(K: int, code_bytes: int) -> np.ndarray:
    if code_bytes == 1:
        return np.arange(K, 256, dtype=np.int64)
    if code_bytes == 2:
        return np.array([-1, -K, -32768, K, 32767], dtype=np.int64)
    return np.array([-1, -K, -(1 << 31), K, 1 << 20, (1 << 31) - 1], dtype=np.int64)


class Case:
    """The arrays of one grid case (built once, read-only)."""

    def __init__(self, spec: Spec):
        self.spec = s = spec
        rng = np.random.default_rng(zlib.crc32(s.name.encode()))
        n, K, F, ldx = s.n, s.K, s.F, s.ldx
        self.tile_rows, self.order = tables(K, s.models)
        self.n_entries = len(self.order)
        order = self.order
        bad = _invalid_codes(K, s.code_bytes)
        if s.dist == "one":
            c = np.full(n, K // 2, dtype=np.int64)
        elif s.dist == "robin":
            c = np.arange(n, dtype=np.int64) % K
        elif s.dist == "random":
            c = rng.integers(0, K, n)
        elif s.dist == "absent":  # first, middle and last code, and first, middle and last entry
            gone = {0, K // 2, K - 1}
            if len(order):
                gone |= {int(order[0]), int(order[len(order) // 2]), int(order[-1])}
            keep = np.array([k for k in range(K) if k not in gone], dtype=np.int64)
            assert len(keep) >= 2
            c = keep[rng.integers(0, len(keep), n)]
        elif s.dist == "heavy":
            c = np.where(rng.random(n) < 0.9, K // 3, rng.integers(0, K, n))
        elif s.dist == "invalid":
            assert len(bad)
            c = bad[rng.integers(0, len(bad), n)]
        elif s.dist == "exact":  # counts: tile_rows, tile_rows + 1, 1, 2 * tile_rows; the rest invalid
            t = self.tile_rows
            c = np.concatenate([np.full(t[0], 0), np.full(t[1] + 1, 1), np.full(1, 2), np.full(2 * t[3], 3)])
            c = c.astype(np.int64)
            assert K == 4 and len(c) <= n and len(bad)
            c = rng.permutation(np.concatenate([c, bad[rng.integers(0, len(bad), n - len(c))]]))
        else:
            raise ValueError(s.dist)
        if s.dist not in ("invalid", "exact") and s.inv_share > 0 and len(bad):
            at = rng.random(n) < s.inv_share
            c = np.where(at, bad[rng.integers(0, len(bad), n)], c)
        self.codes = c.astype(CODE_DTYPES[s.code_bytes])
        assert np.array_equal(self.codes.astype(np.int64), c)  # every code is expressible in its width
        X = rng.integers(-1000, 1000, (n, ldx)).astype(np.float32).view(np.uint32)
        sp = rng.random((n, ldx)) < 0.25
        X[sp] = SPECIAL_BITS[rng.integers(0, len(SPECIAL_BITS), int(sp.sum()))]
        X[:, 0] = np.arange(n, dtype=np.float32).view(np.uint32)
        X[:, F:] = (PAD32 | (np.arange(n, dtype=np.uint32) & np.uint32(0xFFFF)))[:, None]
        self.X = X  # [n, ldx] uint32 bit patterns of the fp32 rows
        self.sg = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)  # ungroup's grouped scores (bits)
        self.vg = rng.integers(0, 256, n).astype(np.uint8)
        for a in (self.codes, self.X, self.sg, self.vg, self.tile_rows, self.order):
            a.setflags(write=False)

    # what the issue's coverage tally asks of the grid
    @property
    def count_workgroups(self) -> int:
        return -(-self.spec.n // COUNT_ROWS)

    def entry_counts(self) -> np.ndarray:
        c = self.codes.astype(np.int64)
        ok = (c >= 0) & (c < self.spec.K)
        counts = np.bincount(c[ok], minlength=self.spec.K)
        return counts[self.order] if self.n_entries else np.zeros(0, np.int64)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return Case(GRID[NAMES.index(name)])


# --------------------------------------------------------------------------- the reference


def _codes(codes: np.ndarray, mutant: Optional[str]) -> np.ndarray:
    if mutant == "codes-u16":
        return codes.astype(np.uint16).astype(np.int64)
    return codes.astype(np.int64)


def _prefix(counts: np.ndarray, mutant: Optional[str]) -> np.ndarray:
    """Exclusive prefix ``[len + 1]`` of ``counts`` (the last element is the total)."""
    out = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=out[1:])
    if mutant == "inclusive-prefix":
        out[:-1] = out[1:]
    return out


def _place(X: np.ndarray, F: int, c: np.ndarray, placed: np.ndarray, starts: np.ndarray, mutant: Optional[str]):
    """Rows ``placed`` in arrival order behind their codes' ``starts``: ``(flat Xg with GUARD words
    of tail, slot of every row or -1, cursor afterwards)``."""
    n, ldx = X.shape
    flat = np.full(n * F + GUARD, GUARD32, dtype=np.uint32)
    slot = np.full(n, -1, dtype=np.int64)
    rows = np.flatnonzero(placed)
    k = c[rows]
    counts = np.bincount(k, minlength=len(starts) - 1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    srt = np.argsort(k, kind="stable")
    rank = np.empty(len(rows), dtype=np.int64)
    rank[srt] = np.arange(len(rows)) - first[k[srt]]  # the row's number among its code's rows, arrival order
    if mutant == "shared-slot":
        rank = np.maximum(rank - 1, 0)
    pos = starts[k] + rank
    if mutant == "slot-off-by-one":
        pos = pos + 1
    slot[rows] = pos
    width = ldx if mutant == "pad-copied" else F
    slow = np.ones(len(rows), dtype=bool)
    if width == F:  # whole slots inside Xg at once (arrival order: of two rows in one slot the later one stays)
        slow = pos >= n
        flat[: n * F].reshape(n, F)[pos[~slow]] = X[rows[~slow], :F]
    for r, p in zip(rows[slow].tolist(), pos[slow].tolist()):  # arrival order, word by word into the flat buffer
        w = min(width, len(flat) - p * F)
        if w > 0:
            flat[p * F: p * F + w] = X[r, :w]
    return flat, slot, starts[:-1] + counts


def ref_group_rows(X, ldx: int, F: int, codes, K: int, mutant: Optional[str] = None, _flat: bool = False):
    """``pmml_group_rows``: ``(starts[K + 1], Xg[n, F], inv[n])``. ``starts`` is the exclusive prefix
    of the per-code counts (what the host hands the kernel as ``cursor``); row ``r`` of a code in
    ``[0, K)`` goes to ``inv[r]`` inside its code's range, any other row gets ``inv[r] = -1``; rows of
    ``Xg`` nothing is placed at keep the guard value. ``X`` is ``[n, ldx]`` (fp32 or its uint32 bits)."""
    X = np.ascontiguousarray(X).view(np.uint32).reshape(len(codes), ldx)
    c = _codes(np.asarray(codes), mutant)
    ok = (c >= 0) & (c < K)
    starts = _prefix(np.bincount(c[ok], minlength=K), mutant)
    flat, inv, cursor = _place(X, F, c, ok, starts, mutant)
    if _flat:
        return starts, flat, inv, cursor
    return starts, flat[: len(c) * F].reshape(len(c), F), inv


def ref_ungroup(sg, vg, inv, mutant: Optional[str] = None):
    """``pmml_ungroup``: ``(score, valid)`` in arrival order — ``sg[inv[j]]`` / ``vg[inv[j]]`` bit for
    bit, NaN / 0 where ``inv[j] == -1``. ``sg`` as fp32 or uint32 bits; the score comes back as bits."""
    sg = np.asarray(sg).view(np.uint32)
    vg = np.asarray(vg, dtype=np.uint8)
    inv = np.asarray(inv, dtype=np.int64)
    src = np.arange(len(inv)) if mutant == "ungroup-no-gather" else np.maximum(inv, 0)
    return np.where(inv >= 0, sg[src], NAN32).astype(np.uint32), np.where(inv >= 0, vg[src], 0).astype(np.uint8)


def ref_group_slice(X, codes, K: int, tile_rows, order, F: Optional[int] = None, mutant: Optional[str] = None,
                    _flat: bool = False):
    """``pmml_group_slice``: ``(row_start[K + 1], tile_start[n_entries + 1], cursor afterwards,
    Xg[n, F], perm[n], out_s[n], out_v[n])``. Only codes with ``tile_rows > 0`` have a model: their
    rows are counted (``row_start``: exclusive prefix by code) and placed (``perm[pos]`` = arrival
    row), the entries' tiles ``ceil(count / tile_rows)`` are numbered in ``order`` (``tile_start``);
    every other row is answered NaN / 0 at its arrival index. Untouched elements keep the guard."""
    codes = np.asarray(codes)
    n = len(codes)
    X = np.ascontiguousarray(X).view(np.uint32).reshape(n, -1)
    F = X.shape[1] if F is None else F
    tile_rows = np.asarray(tile_rows, dtype=np.int64)
    order = np.asarray(order, dtype=np.int64)
    c = _codes(codes, mutant)
    ok = (c >= 0) & (c < K)
    has = ok.copy()
    has[ok] = tile_rows[c[ok]] > 0
    counted = ok if mutant == "no-model-counted" else has
    counts = np.bincount(c[counted], minlength=K)
    row_start = _prefix(counts, mutant)
    tr = np.maximum(tile_rows, 1)
    tiles = counts // tr if mutant == "tiles-floor" else -(-counts // tr)
    tiles = np.where(tile_rows > 0, tiles, 0)
    by_entry = tiles[np.sort(order)] if mutant == "tiles-code-order" else tiles[order]
    tile_start = _prefix(by_entry, mutant)
    flat, slot, cursor = _place(X, F, c, has, row_start, mutant)
    perm = np.full(n, GUARD32.view(np.int32), dtype=np.int64)
    at = np.flatnonzero(has)
    inside = slot[at] < n
    perm[slot[at][inside]] = at[inside]
    out_s = np.full(n, GUARD32, dtype=np.uint32)
    out_v = np.full(n, GUARD8, dtype=np.uint8)
    if mutant != "invalid-unanswered":
        out_s[~has], out_v[~has] = NAN32, 0
    Xg = flat if _flat else flat[: n * F].reshape(n, F)
    return row_start, tile_start, cursor, Xg, perm, out_s, out_v


# --------------------------------------------------------------------------- buffers


def guarded(words: int, dtype=np.uint32, off: int = 0) -> np.ndarray:
    """A buffer of ``GUARD + off + words + GUARD`` elements, every one the guard value."""
    fill = GUARD8 if np.dtype(dtype).itemsize == 1 else GUARD32.view(dtype)
    return np.full(GUARD + off + words + GUARD, fill, dtype=dtype)


def body(buf: np.ndarray, words: int, off: int = 0) -> np.ndarray:
    assert len(buf) == GUARD + off + words + GUARD, (len(buf), words, off)
    return buf[GUARD + off: GUARD + off + words]


def _filled(values, dtype, off: int = 0, tail=None) -> np.ndarray:
    values = np.asarray(values)
    buf = guarded(len(values), dtype, off)
    body(buf, len(values), off)[:] = values.astype(dtype) if values.dtype != dtype else values
    if tail is not None:
        buf[len(buf) - GUARD:] = tail
    return buf


def emulate_group_rows(cs: Case, mutant: Optional[str] = None) -> Dict[str, np.ndarray]:
    s = cs.spec
    _, flat, inv, cursor = ref_group_rows(cs.X, s.ldx, s.F, cs.codes, s.K, mutant, _flat=True)
    nF = s.n * s.F
    return dict(Xg=_filled(flat[:nF], np.uint32, s.xg_off, tail=flat[nF:]), inv=_filled(inv, np.int32),
                cursor=_filled(cursor, np.int32))


def emulate_ungroup(cs: Case, inv: np.ndarray, mutant: Optional[str] = None, second: bool = True):
    sc, va = ref_ungroup(cs.sg, cs.vg, inv, mutant)
    out = dict(out_s=_filled(sc, np.uint32), out_v=_filled(va, np.uint8))
    if second:
        skip = mutant == "second-pair-skipped"
        out["out_s2"] = guarded(len(sc), np.uint32) if skip else _filled(sc, np.uint32)
        out["out_v2"] = guarded(len(va), np.uint8) if skip else _filled(va, np.uint8)
    return out


def emulate_group_slice(cs: Case, mutant: Optional[str] = None) -> Dict[str, np.ndarray]:
    s = cs.spec
    row_start, tile_start, cursor, flat, perm, out_s, out_v = ref_group_slice(
        cs.X, cs.codes, s.K, cs.tile_rows, cs.order, F=s.F, mutant=mutant, _flat=True)
    nF = s.n * s.F
    counts = np.diff(row_start) if mutant == "counts-not-cleared" else np.zeros(s.K, np.int64)
    ticket = cs.count_workgroups if mutant == "ticket-not-reset" else 0
    return dict(Xg=_filled(flat[:nF], np.uint32, s.xg_off, tail=flat[nF:]), perm=_filled(perm, np.int32),
                out_s=_filled(out_s, np.uint32), out_v=_filled(out_v, np.uint8), cursor=_filled(cursor, np.int32),
                row_start=_filled(row_start, np.int32), tile_start=_filled(tile_start, np.int32),
                counts=_filled(counts, np.int32), ticket=_filled([ticket], np.int32))


# --------------------------------------------------------------------------- the order-free checker

G32I = int(GUARD32.view(np.int32))


def _guards(name: str, what: str, buf: np.ndarray, words: int, off: int = 0) -> np.ndarray:
    b = body(buf, words, off)
    g = GUARD8 if buf.dtype.itemsize == 1 else GUARD32.view(buf.dtype)
    front, back = buf[: GUARD + off], buf[GUARD + off + words:]
    assert (front == g).all(), f"{name}: guard before {what} overwritten at {np.flatnonzero(front != g)[:4]}"
    assert (back == g).all(), f"{name}: guard behind {what} overwritten at {np.flatnonzero(back != g)[:4]}"
    return b


def _same_rows(name: str, what: str, Xg: np.ndarray, pos: np.ndarray, X: np.ndarray, rows: np.ndarray, F: int) -> None:
    diff = np.flatnonzero((Xg[pos] != X[rows, :F]).any(axis=1))
    if len(diff):
        i = diff[0]
        got = Xg[pos[i], 0].view(np.float32)
        raise AssertionError(f"{name}: {what}: slot {int(pos[i])} should hold row {int(rows[i])} bit for bit and holds "
                             f"{Xg[pos[i]]} (column 0 names row {got}); {len(diff)} slots differ")


def _bijection(name: str, what: str, v: np.ndarray, size: int) -> None:
    seen = np.bincount(v, minlength=size) if len(v) else np.zeros(size, np.int64)
    assert len(seen) == size and (seen == 1).all(), \
        f"{name}: {what} is no bijection onto [0, {size}): {int((seen > 1).sum())} values shared, " \
        f"{int((seen[:size] == 0).sum())} unused (first shared {np.flatnonzero(seen > 1)[:3]})"


def check_group_rows(cs: Case, out: Dict[str, np.ndarray]) -> None:
    s, name = cs.spec, cs.spec.name
    n, K, F = s.n, s.K, s.F
    c = cs.codes.astype(np.int64)
    ok = (c >= 0) & (c < K)
    starts = np.concatenate([[0], np.cumsum(np.bincount(c[ok], minlength=K))])
    n_valid = int(starts[K])
    inv = _guards(name, "inv", out["inv"], n).astype(np.int64)
    Xg = _guards(name, "Xg", out["Xg"], n * F, s.xg_off).reshape(n, F)
    cursor = _guards(name, "cursor", out["cursor"], K)
    wrong = np.flatnonzero((inv == -1) != ~ok)
    assert len(wrong) == 0, (f"{name}: inv == -1 exactly for codes outside [0, {K}): row {wrong[0]}, "
                             f"code {c[wrong[0]]}, inv {inv[wrong[0]]}")
    rows = np.flatnonzero(ok)
    v = inv[rows]
    off = np.flatnonzero((v < starts[c[rows]]) | (v >= starts[c[rows] + 1]))
    assert len(off) == 0, (f"{name}: row {rows[off[0]]} of code {c[rows[off[0]]]} at slot {v[off[0]]}, outside "
                           f"[{starts[c[rows[off[0]]]]}, {starts[c[rows[off[0]]] + 1]}); {len(off)} rows")
    _bijection(name, "inv over the valid rows", v, n_valid)
    _same_rows(name, "group_rows", Xg, v, cs.X, rows, F)
    assert (Xg[n_valid:] == GUARD32).all(), f"{name}: rows of Xg past the {n_valid} grouped rows were written"
    assert np.array_equal(cursor, starts[1:]), f"{name}: cursor afterwards is not starts[1:]"


def check_ungroup(cs: Case, inv: np.ndarray, out: Dict[str, np.ndarray]) -> None:
    """``inv``: the inverse permutation the outputs were gathered through (already checked)."""
    name, n = cs.spec.name, cs.spec.n
    inv = np.asarray(inv, dtype=np.int64)
    at = np.maximum(inv, 0)
    pairs = [("out_s", "out_v")] + ([("out_s2", "out_v2")] if "out_s2" in out else [])
    for ks, kv in pairs:
        sc = _guards(name, ks, out[ks], n)
        va = _guards(name, kv, out[kv], n)
        ok = inv >= 0
        bad = np.flatnonzero(ok & ((sc != cs.sg[at]) | (va != cs.vg[at])))
        assert len(bad) == 0, (f"{name}: {ks}[{bad[0]}] = {sc[bad[0]]:#x} / {kv} = {va[bad[0]]}, want "
                               f"sg[{inv[bad[0]]}] = {cs.sg[at[bad[0]]]:#x} / {cs.vg[at[bad[0]]]}; {len(bad)} rows")
        assert np.isnan(sc[~ok].view(np.float32)).all() and (va[~ok] == 0).all(), \
            f"{name}: rows with inv == -1 must read NaN / 0 in {ks} / {kv}"


def check_group_slice(cs: Case, out: Dict[str, np.ndarray]) -> None:
    s, name = cs.spec, cs.spec.name
    n, K, F, ne = s.n, s.K, s.F, cs.n_entries
    c = cs.codes.astype(np.int64)
    ok = (c >= 0) & (c < K)
    has = ok.copy()
    has[ok] = cs.tile_rows[c[ok]] > 0
    counts = np.bincount(c[has], minlength=K)
    row_start = np.concatenate([[0], np.cumsum(counts)])
    total = int(row_start[K])
    tr = cs.tile_rows[cs.order[:ne]].astype(np.int64)
    tile_start = np.concatenate([[0], np.cumsum(-(-counts[cs.order[:ne]] // tr))]).astype(np.int64)
    got_counts = _guards(name, "counts", out["counts"], K)
    got_ticket = _guards(name, "ticket", out["ticket"], 1)
    assert (got_counts == 0).all(), f"{name}: counts not all zero afterwards (code {np.flatnonzero(got_counts)[0]})"
    assert got_ticket[0] == 0, f"{name}: ticket is {got_ticket[0]} afterwards, not 0"
    got = _guards(name, "row_start", out["row_start"], K + 1)
    assert np.array_equal(got, row_start), \
        f"{name}: row_start differs first at code {np.flatnonzero(got != row_start)[0]} (total {got[K]} for {total})"
    got = _guards(name, "tile_start", out["tile_start"], ne + 1)
    assert np.array_equal(got, tile_start), (f"{name}: tile_start differs first at entry "
                                             f"{np.flatnonzero(got != tile_start)[0]} ({got[ne]} tiles for {tile_start[ne]})")
    got = _guards(name, "cursor", out["cursor"], K)
    assert np.array_equal(got, row_start[1:]), f"{name}: cursor afterwards is not row_start[1:]"
    perm = _guards(name, "perm", out["perm"], n).astype(np.int64)
    Xg = _guards(name, "Xg", out["Xg"], n * F, s.xg_off).reshape(n, F)
    p = perm[:total]
    assert ((p >= 0) & (p < n)).all(), f"{name}: perm holds {p[(p < 0) | (p >= n)][:3]}, not rows of the slice"
    assert has[p].all(), f"{name}: perm names row {p[~has[p]][0]}, which has no model"
    _bijection(name, "perm as a map onto the rows with a model", np.cumsum(has)[p] - 1, total)
    pos = np.arange(total)
    off = np.flatnonzero((pos < row_start[c[p]]) | (pos >= row_start[c[p] + 1]))
    assert len(off) == 0, f"{name}: slot {off[:1]} holds row {p[off[:1]]}, outside its code's range; {len(off)} slots"
    assert (perm[total:] == G32I).all(), f"{name}: perm written past the {total} grouped rows"
    _same_rows(name, "group_slice", Xg, pos, cs.X, p, F)
    assert (Xg[total:] == GUARD32).all(), f"{name}: rows of Xg past the {total} grouped rows were written"
    sc = _guards(name, "out_s", out["out_s"], n)
    va = _guards(name, "out_v", out["out_v"], n)
    assert np.isnan(sc[~has].view(np.float32)).all() and (va[~has] == 0).all(), \
        f"{name}: a row without a model is not answered NaN / 0 at its arrival index"
    assert (sc[has] == GUARD32).all() and (va[has] == GUARD8).all(), \
        f"{name}: out_s / out_v written at a row that has a model (the tree launch answers those)"


def failures(cs: Case, mutant: Optional[str]) -> List[str]:
    """The checks the emulated buffers of ``mutant`` (``None``: the reference) fail, by entry point."""
    found = []
    rows = emulate_group_rows(cs, mutant)
    inv = body(ref_buffers(cs)["inv"], cs.spec.n)  # ungroup gathers through the true inverse permutation
    for what, fn in (("group_rows", lambda: check_group_rows(cs, rows)),
                     ("ungroup", lambda: check_ungroup(cs, inv, emulate_ungroup(cs, inv, mutant))),
                     ("ungroup-1", lambda: check_ungroup(cs, inv, emulate_ungroup(cs, inv, mutant, second=False))),
                     ("group_slice", lambda: check_group_slice(cs, emulate_group_slice(cs, mutant)))):
        try:
            fn()
        except AssertionError as e:
            found.append(f"{what}: {e}")
    return found


@functools.lru_cache(maxsize=None)
def _ref_buffers(name: str):
    return emulate_group_rows(case(name))


def ref_buffers(cs: Case):
    return _ref_buffers(cs.spec.name)


# --------------------------------------------------------------------------- the grouped tree launch

FLEET_F = 8
FLEET_ROWS = 5000
FLEET_SLICE = 1024  # rows per slice: 5000 rows make five slices through one ring and one set of tables
# (depth, trees, seed, field preparation) of the tree models, in code order with the two scorers
# without a model between them: codes 0..3 one launch group, 5..7 the other
FLEET = [(4, 5, 41, False), (4, 9, 42, True), (4, 7, 43, False), (4, 3, 44, False), "null",
         (6, 4, 45, False), (6, 6, 46, False), (6, 5, 47, False), "unknown"]
FLEET_GROUPS = ([0, 1, 2, 3], [5, 6, 7])
PREP_BOUNDS = {1: [-5.0, 0.3], 2: [-5.0, 0.7]}


@functools.lru_cache(maxsize=None)
def fleet_documents() -> tuple:
    """The GBDT regression documents of ``FLEET`` (``None`` for the two codes without a model):
    integer leaves, so every sum is exact in fp32; model 1 prepares two of its fields (an interval
    with ``asValue`` and one with ``returnInvalid``: some of its rows are invalid)."""
    from flink_jpmml_amd.bench.synth import gbdt_pmml
    from tests import _boundary as B
    from tests import _prep_grid as G

    docs = []
    for m in FLEET:
        if isinstance(m, str):
            docs.append(None)
            continue
        depth, trees, seed, prep = m
        txt = B.integer_leaves(gbdt_pmml(n_trees=trees, depth=depth, n_features=FLEET_F, seed=seed))
        if prep:
            for j, ivt in ((1, "asValue"), (2, "returnInvalid")):
                lo, hi = PREP_BOUNDS[j]
                txt = G.treat_field(txt, j, f'<Interval closure="closedOpen" leftMargin="{lo}" rightMargin="{hi}"/>',
                                    None, "", "float", ivt)
        docs.append(txt)
    return tuple(docs)


@functools.lru_cache(maxsize=None)
def fleet_inputs() -> np.ndarray:
    """Every cell a split cut of some model of the fleet (or a preparation bound) +-2 ulps, or a
    special value: rows sit on the thresholds of the model that scores them."""
    from tests import _boundary as B

    cuts = [set() for _ in range(FLEET_F)]
    for txt in fleet_documents():
        if txt is not None:
            for j, cu in enumerate(B.split_cuts(txt, FLEET_F)):
                cuts[j] |= set(cu)
    for j, b in PREP_BOUNDS.items():
        cuts[j] |= set(b)
    X = B.boundary_matrix([sorted(c) for c in cuts], FLEET_ROWS, seed=17)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def fleet_codes(rows_wide: int = 256) -> np.ndarray:
    """One code per row, slice by slice (``FLEET_SLICE`` rows each). Slice 0: the FIRST entry of the
    first launch group and the LAST entry of the second have no row, one model has exactly
    ``rows_wide`` rows, one ``rows_wide + 1`` and one a single row. Slice 1: the same with the last
    entry of the first group and the first of the second. Slice 3: a middle entry of each group is
    empty. Slices 2 and 4: every code, uniformly."""
    rng = np.random.default_rng(23)
    K = len(FLEET)
    (a0, a1, a2, a3), (b0, b1, b2) = FLEET_GROUPS
    nul, unk = FLEET.index("null"), FLEET.index("unknown")

    def crafted(exact, plus_one, single, rest, m):
        c = np.concatenate([np.full(rows_wide, exact), np.full(rows_wide + 1, plus_one), np.full(1, single)])
        fill = np.array(rest)[np.arange(m - len(c)) % len(rest)]
        return rng.permutation(np.concatenate([c, fill]))

    out = []
    for i, s in enumerate(range(0, FLEET_ROWS, FLEET_SLICE)):
        m = min(FLEET_SLICE, FLEET_ROWS - s)
        if i == 0:
            c = crafted(a1, a2, a3, [b0, b1, nul, unk], m)
        elif i == 1:
            c = crafted(b1, b2, a0, [a1, a2, nul, unk], m)
        elif i == 3:
            c = np.array([a0, a2, a3, b0, b2, nul, unk])[rng.integers(0, 7, m)]
        else:
            c = rng.integers(0, K, m)
        out.append(c)
    codes = np.concatenate(out).astype(np.uint8)
    codes.setflags(write=False)
    return codes
