"""CPU side of the GPU CSV parser's pin (``tests/_text_cases.py``): every placement and dispatch
path a case claims holds; the twin's row starts are the lines ``RecordParser`` turns into rows; the
twin's raw matrix with its flagged rows replaced by the host parser's rows IS the host parser's
matrix, bit for bit; every value the twin's fast path accepts is the correctly rounded fp32 of the
decimal (over rationals); and every named mutant of the twin changes ``starts``, ``X_raw`` or the
flag set of a case built to catch it — or is shown to change nothing, with the reason.
``test_gpu_text_kernels.py`` then holds the kernels to the twin."""

import numpy as np
import pytest

from tests import _text_cases as T

ALL = [c["name"] for c in T.all_cases()]
ROWS = [c["name"] for c in T.row_cases()]


@pytest.fixture(scope="module")
def host():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = T.host_parse(T.case_named(name))
        return memo[name]

    return get


# --------------------------------------------------------------------------- claims


def test_every_table_is_present_and_names_are_unique():
    assert len(set(ALL)) == len(ALL)
    for at in T.START_PLACEMENTS:
        assert f"start@{at}" in ALL
    for m in T.CAPACITIES:
        assert f"capacity-{m}" in ALL
    assert {"tiles-1025", "tiles-2051", "dense-3-tiles", "newline", "seven", "only-empty-lines"} <= set(ALL)


@pytest.mark.parametrize("name", ROWS)
def test_row_start_placements(name):
    c = T.case_named(name)
    buf, claims = c["buf"], c["claims"]
    n = len(buf)
    starts = T.twin_row_starts(buf)
    s = set(starts.tolist())
    for at in claims.get("start_at", []):
        assert at in s and (at == 0 or buf[at - 1] == 10), (name, at)
    if name.startswith("start@"):
        at = int(name.split("@")[1])
        assert claims["start_at"][0] == at
        assert claims["start_at"][1] == n - 2 == int(starts[-1]) and buf[-2:] == b"7\n"
    if "crlf_at" in claims:
        at = claims["crlf_at"]
        assert buf[at - 1: at + 2] == b"\n\r\n" and at not in s and at + 1 not in s and at + 2 in s
        assert (at + 1) % 16 == 0 and at + 1 in (16, 1024, 4096)
        assert at in set(T.twin_row_starts(buf, "crlf-line-not-empty").tolist())
    if "empty_run" in claims:
        lo, hi = claims["empty_run"]
        run = buf[lo:hi]
        assert lo < 4096 < hi and set(run) == {10, 13} and run.count(b"\n") == 40 and 0 < run.count(b"\r") < 40
        assert not any(lo <= x < hi for x in s) and claims["start_at"][0] == hi
    if name == "only-empty-lines":
        assert len(starts) == 0 and n > T.TILE and b"\r\n" in buf
    if name == "newline":
        assert buf == b"\n" and len(starts) == 0
    if name == "seven":
        assert buf == b"7\n" and starts.tolist() == [0]
    tile_counts = np.bincount(starts // T.TILE, minlength=-(-n // T.TILE))
    if "per_tile" in claims:  # 8 starts in every 16-byte lane, 2048 in every tile
        assert n == 3 * T.TILE and (tile_counts == claims["per_tile"]).all()
        assert (np.bincount(starts // 16, minlength=n // 16) == 8).all()
    for t in claims.get("empty_tiles", []):
        assert tile_counts[t] == 0 and tile_counts[t + 1] > 0
    if "n_tiles" in claims:
        tiles = claims["n_tiles"]
        assert len(tile_counts) == tiles and n < 9_000_000 and n % T.TILE
        per = -(-tiles // 1024)  # row_start_scan: tiles per thread
        assert per == {1025: 2, 2051: 3}[tiles]
        assert 1023 * per > tiles  # the trailing threads' ranges are empty
        assert (tile_counts == T.TILE // 2).sum() >= 5 and (tile_counts == 0).sum() >= 100
        assert ((tile_counts > 0) & (tile_counts < T.TILE // 2)).sum() >= 100
        assert len(starts) < 2 ** 24  # the identifying payloads are exact in fp32


def test_dispatch_reference_numbers():
    """The LDS arithmetic at the sizes where it changes: the cap limits and the F at which the
    output tile alone no longer leaves room for 4 KiB of text."""
    big = 1 << 30
    assert T.twin_lds(big, 1, 200)[:2] == (True, 58864)
    assert T.twin_lds(big, 1, 256)[:2] == (True, 30192)
    assert T.twin_lds(big, 1, 306)[:2] == (True, 4592)
    assert T.twin_lds(big, 1, 307)[0] is False
    assert T.twin_lds(100, 10, 4) == (True, 4096, T.PR_TB * 5 * 4 + 4096 + 16)  # the 4 KiB floor
    assert all(T.twin_lds(big, 1, F)[2] <= 160 * 1024 - 2048 for F in range(1, 307))
    assert T.twin_dispatch(0, 0, 1, 1, True, []) == []


@pytest.mark.parametrize("name", [c["name"] for c in T.dispatch_cases()])
def test_dispatch_cases_reach_their_paths(name):
    c = T.case_named(name)
    starts = T.twin_of(name)[0]
    groups = T.twin_dispatch(len(c["buf"]), len(starts), c["n_cols"], c["F"], c["misalign"] % 16 == 0, starts)
    claims = c["claims"]
    assert set(groups) == claims["paths"], (name, groups)
    if "groups" in claims:
        assert groups == claims["groups"]
    if claims.get("lds_over_64k"):
        assert T.twin_lds(len(c["buf"]), len(starts), c["F"])[2] > 65536
    else:
        assert "lds" not in claims["paths"] or T.twin_lds(len(c["buf"]), len(starts), c["F"])[2] <= 65536
    if "n_rows" in claims:
        assert len(starts) == claims["n_rows"] and len(starts) % T.PR_TB == 1
    if name == "global-misaligned":
        assert c["misalign"] == 1
        assert set(T.twin_dispatch(len(c["buf"]), len(starts), c["n_cols"], c["F"], True, starts)) == {"lds"}
    if name == "global-257-columns":
        assert set(T.twin_dispatch(len(c["buf"]), len(starts), 256, c["F"], True, starts)) == {"lds"}
    if name == "global-F307":
        assert "global-kernel" not in T.twin_dispatch(len(c["buf"]), len(starts), 256, 306, True, starts)
    if name == "lds-fallback-long-field":
        line5 = c["buf"][starts[5]: starts[6]]
        assert len(line5.split(b",")[3]) == 65536 and T.SIX_COLMAP[3] == -1


def test_every_other_case_takes_the_lds_kernel():
    for c in T.all_cases():
        if c in T.dispatch_cases() or c["misalign"]:
            continue
        starts = T.twin_of(c["name"])[0]
        groups = T.twin_dispatch(len(c["buf"]), len(starts), c["n_cols"], c["F"], True, starts)
        if "n_tiles" in c["claims"]:  # workgroups of 5000-byte lines exceed the chunk's average
            assert set(groups) == {"lds", "lds-fallback"} and groups.count("lds-fallback") >= 10
        else:
            assert set(groups) == ({"lds"} if len(starts) else set()), (c["name"], set(groups))


def test_capacity_buffer_has_exactly_five_flagged_records():
    for c in T.capacity_cases():
        starts, _, flagged = T.twin_of(c["name"])
        assert len(starts) == 300 and flagged.tolist() == list(T.CAPACITY_ROWS) == c["claims"]["flagged_rows"]
        assert len({r // T.PR_TB for r in T.CAPACITY_ROWS}) == 3  # every workgroup flags
    assert [c["max_flagged"] for c in T.capacity_cases()] == [0, 4, 5, 6, 64]


def test_missing_tables():
    c8, cdef, cempty = T.missing_cases()
    assert len(c8["missing"]) == T.MAX_MISSING and len(cempty["missing"]) == 0
    assert sum(len(m) == T.MISSING_LEN - 1 for m in c8["missing"]) == 1
    toks = c8["claims"]["tokens"]
    miss = [m.encode() for m in c8["missing"]]
    assert any(any(m.startswith(t) and m != t for m in miss) for t in toks if t)  # strict prefixes
    assert any(any(t.startswith(m) and m != t for m in miss) for t in toks)  # extensions
    assert any(any(t.lower() == m.lower() and m != t for m in miss) for t in toks)  # letter case only
    assert b"missing_value_xy" in toks and len(b"missing_value_xy") == T.MISSING_LEN
    # the table decides: the same buffer flags differently under the three tables
    sets = [set(T.twin_of(c["name"])[2].tolist()) for c in (c8, cdef, cempty)]
    assert sets[0] < sets[1] < sets[2]


# --------------------------------------------------------------------------- twin against the host parser


@pytest.mark.parametrize("name", ROWS)
def test_row_starts_are_the_host_parsers_rows(name, host):
    """Row count, and the identifying payloads in order."""
    c = T.case_named(name)
    starts, X, flagged = T.twin_of(name)
    H = host(name)
    assert H.shape == (len(starts), 1) and len(flagged) == 0
    want = np.array(c["claims"]["values"], dtype=np.float32).reshape(-1, 1)
    assert np.array_equal(T.bits(H), T.bits(want))
    assert np.array_equal(T.bits(X), T.bits(want))


@pytest.mark.parametrize("name", ALL)
def test_patched_twin_equals_host_parser(name, host):
    """``X_raw`` with the flagged rows taken from the host parser equals ``RecordParser.parse``:
    NaN mask and fp32 bits, -0.0 included. Unflagged rows are therefore final as the kernel writes
    them; flagged rows hold NaN exactly where the fast path does not settle a token."""
    starts, X, flagged = T.twin_of(name)
    H = host(name)
    assert H.shape == X.shape, (H.shape, X.shape)
    patched = X.copy()
    patched[flagged] = H[flagged]
    assert T.same_matrix(patched, H), np.argwhere(np.isnan(patched) != np.isnan(H))[:5]
    # what the kernel wrote into a flagged row is either NaN or already the host's value
    raw = X[flagged]
    keep = ~np.isnan(raw)
    assert np.array_equal(T.bits(raw)[keep], T.bits(H[flagged])[keep])
    print(f"{name}: {len(starts)} rows, {len(flagged)} flagged")


def test_pinned_host_spellings(host):
    """Host behaviour at the edges of fp32, pinned as it is (``docs/PARITY.md``): overflow and
    underflow spellings are NaN, ``1e-45`` is the smallest subnormal, the inf spellings the host
    lists are +-inf, ``-0`` keeps its sign."""
    c = T.case_named("tokens-placed")
    H = host("tokens-placed")[:, 0]
    at = {t: i for i, t in enumerate(c["claims"]["tokens"])}
    for t in (b"1e400", b"3.5e38", b"1e-46", b"nan(abc)", b"1_0", b"0x10", b"\r5", b"1e", b"+.", b"--1"):
        assert np.isnan(H[at[t]]), t
    assert T.bits(H[at[b"1e-45"]]) == 1
    assert H[at[b"inf"]] == np.inf and H[at[b"Infinity"]] == np.inf and H[at[b"-inf"]] == -np.inf
    assert H[at[b"INF"]] == np.inf and H[at[b"+inf"]] == np.inf
    assert T.bits(H[at[b"-0"]]) == 0x80000000 == T.bits(H[at[b"-0.0"]]) and T.bits(H[at[b"0e99999"]]) == 0
    assert np.isnan(H[at[b" \r 5 \r"]])  # a '\r' is trimmed at the end of a token only
    assert H[at[b"1e0000001"]] == 10.0 and H[at[b"1e000001"]] == 10.0
    assert H[at[b"5 \r\t\""]] == 5.0 and H[at[b"5\r"]] == 5.0 and H[at[b"-.5"]] == -0.5 and H[at[b"5."]] == 5.0


# --------------------------------------------------------------------------- fast path against rationals


def test_fast_path_is_correct_rounding_and_settles_most_tokens():
    shares = {}
    for c in T.token_cases() + T.missing_cases()[1:2]:
        starts, X, flagged = T.twin_of(c["name"])
        toks = c["claims"]["tokens"]
        assert len(toks) == len(starts)  # one record per token
        fl = set(flagged.tolist())
        accepted = 0
        for r, tok in enumerate(toks):
            s, e = T.twin_trim(tok, 0, len(tok))
            t = tok[s:e]
            if not t or t.decode("latin-1") in c["missing"]:
                assert r not in fl and np.isnan(X[r, 0]), tok
                continue
            v = T.twin_fast_token(t)
            assert (v is None) == (r in fl), tok
            if v is None:
                assert np.isnan(X[r, 0]), tok
                continue
            accepted += 1
            assert T.bits(v) == T.bits(X[r, 0]) == T.bits(T.f32_correctly_rounded(t)), tok
            assert T.bits(X[r, 1]) == 0
        shares[c["name"]] = (len(fl), len(toks), accepted)
    print(shares)
    k, n, accepted = shares["tokens-generated"]
    assert n > 5900 and accepted > 3000
    assert k < 0.40 * n, f"{k} of {n} generated tokens flagged: the fast path is what is under test"


def test_placed_token_edges_fall_where_they_are_meant_to():
    fast = lambda t: T.twin_fast_token(t) is not None  # noqa: E731
    d19, d20 = b"1234567890123456789", b"12345678901234567890"
    # 19 digits pass the digit count but exceed 2^53; 20 digits stop at the count, before w (which
    # wraps at 2^64: 2^64 + 1 would otherwise read as 1) is looked at
    assert not fast(d19) and not fast(d20) and not fast(b"0" * 25 + d19) and not fast(b"9" * 19)
    assert not fast(b"18446744073709551617") and fast(b"1") and (18446744073709551617 * 10 // 10) & T.M64 == 1
    w53 = b"%d" % 2 ** 53
    assert fast(w53) and fast(b"0" * 25 + w53) and fast(b"0.000" + w53) and len(b"0000" + w53) == 20
    assert not fast(w53 + b"0000")  # 20 significant digits
    assert fast(b"%d" % (2 ** 53 - 1)) and fast(b"%d" % 2 ** 53) and not fast(b"%d" % (2 ** 53 + 1))
    assert fast(b"9.007199254740992") and not fast(b"9.007199254740993")
    assert fast(b"1e22") and not fast(b"1e23") and fast(b"1e-22") and not fast(b"1e-23")
    assert fast(b"123.456e20") and fast(b"123.456e25") and not fast(b"123.456e26")
    assert fast(b"0." + b"0" * 21 + b"1") and not fast(b"0." + b"0" * 22 + b"1")
    assert fast(b"1e000001") and not fast(b"1e0000001")
    for t in (b"1e", b"1e+", b"1e-", b"e5", b".", b"+.", b"+", b"-", b"--1", b"+-1", b"inf", b"1_0", b"0x10"):
        assert not fast(t), t
    assert T.bits(T.twin_fast_token(b"-0")) == 0x80000000 and T.bits(T.twin_fast_token(b"0e22")) == 0
    assert not fast(b"0e99999") and not fast(b"0e23")  # the exponent limit comes before the value
    assert fast(b"-.5") and fast(b"5.") and fast(b"+5")
    mid = [b"%d.5" % k for k in range(2 ** 23, 2 ** 23 + 300)] + [b"%d" % k for k in range(2 ** 24 + 1, 2 ** 24 + 100, 2)]
    assert not any(fast(t) for t in mid)
    assert all(fast(b"%d.4" % k) and fast(b"%d.6" % k) for k in range(2 ** 23, 2 ** 23 + 300))
    assert all(fast(b"%d" % (k - 1)) and fast(b"%d" % (k + 1)) for k in range(2 ** 24 + 1, 2 ** 24 + 100, 2))
    # |exp10| <= 22 keeps every non-zero fast-path value at or above 1e-22: the subnormal branch of
    # finish_decimal is reached with d == 0 only
    assert not fast(b"1e-40") and not fast(b"1.17549435e-38") and fast(b"0.0000000000000000000001")
    placed = set(T.placed_tokens())
    assert {d19, d20, b"1e23", b"1e0000001", b"8388608.5", b"16777217", b"1\x805", b"1\x005", b" \r 5 \r"} <= placed


# --------------------------------------------------------------------------- mutants

CATCHES = {
    "no-midpoint-test": ["tokens-placed", "tokens-generated", "capacity-5"],
    "w-ge-2^53": ["tokens-placed"],
    "digits-count-leading-zeros": ["tokens-placed"],
    "digits-limit-20": ["tokens-placed"],
    "exp10-limit-23": ["tokens-placed", "tokens-generated"],
    "exponent-7-digits": ["tokens-placed"],
    "cr-trimmed-at-front": ["tokens-placed"],
    "missing-matched-as-prefix": ["missing-8-tokens", "missing-default"],
    "crlf-line-not-empty": ["crlf@15", "crlf@1023", "crlf@4095", "empty-run@4096", "only-empty-lines", "shapes-comma"],
    "no-start-at-byte-0": ["start@0", "seven", "dense-3-tiles", "long-line-then-short", "tokens-placed"],
}


def _changed(a, b) -> bool:
    (s0, x0, f0), (s1, x1, f1) = a, b
    return not (np.array_equal(s0, s1) and T.same_matrix(x0, x1) and np.array_equal(f0, f1))


def test_mutant_table_is_complete():
    assert set(CATCHES) | set(T.INERT_MUTANTS) == set(T.MUTANTS) == set(T.MUTANT_FUNCS)
    assert not set(CATCHES) & set(T.INERT_MUTANTS)


@pytest.mark.parametrize("mutant", list(CATCHES))
def test_named_mutants_show(mutant):
    """A rule restated wrongly must show on the cases meant to catch it: a mutant no case detects
    means the cases are too weak, not that the kernel is right."""
    for name in CATCHES[mutant]:
        assert _changed(T.twin_of(name), T.MUTANT_FUNCS[mutant](T.case_named(name))), (mutant, name)


@pytest.mark.parametrize("mutant", T.INERT_MUTANTS)
def test_inert_mutants_change_nothing(mutant):
    """``no-ragged-break``: dropping ``if (te >= le) break;`` cannot show. ``te`` stops at ``le``,
    so the next statement sets ``p = le + 1`` and the loop's own guard ``p <= le`` ends it before
    another column is read. Demonstrated on every case, ragged rows and trailing delimiters
    included."""
    ragged = 0
    for c in T.all_cases():
        if "n_tiles" in c["claims"]:  # one column: the loop ends on `c < n_cols` whatever the break does
            continue
        assert not _changed(T.twin_of(c["name"]), T.MUTANT_FUNCS[mutant](c)), (mutant, c["name"])
        if c["n_cols"] > 1:
            ragged += sum(line.count(c["delim"]) < c["n_cols"] - 1 for line in c["buf"].split(b"\n") if line)
    assert ragged > 500
