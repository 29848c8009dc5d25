"""The GPU CSV parser's kernels (``ops/csrc/textparse.hip``) held to their twin
(``tests/_text_cases.py``) before any host patching: the row starts, the raw matrix the parse
kernels write (flagged rows included), the flag counter and the flag list, with guard elements
behind every output. Every comparison is exact. ``test_text_cases.py`` proves on the CPU that the
twin, patched with the host parser's rows, is the host parser, and that each case sits where it
claims to. Then the reader level: ``DeviceTextReader`` over files written from the case buffers,
around the ``k > max_flagged`` whole-chunk branch, bit-identical to ``native.RecordParser``."""

import numpy as np
import pytest

from tests import _text_cases as T

pytestmark = pytest.mark.gpu

ALL = [c["name"] for c in T.all_cases()]


@pytest.fixture(scope="module")
def lib(gpu):
    from flink_jpmml_amd.ops import _lib

    return _lib.load()


def _run(lib, gpu, c, **over):
    a = dict(c, **over)
    return T.device_parse(lib, gpu, a["buf"], a["n_cols"], a["colmap"], a["F"], a["delim"], a["missing"],
                          a["max_flagged"], misalign=a["misalign"])


@pytest.mark.parametrize("name", ALL)
def test_kernels_equal_twin(gpu, lib, name):
    c = T.case_named(name)
    starts, X, flagged = T.twin_of(name)
    got = _run(lib, gpu, c)
    assert got["rc"] == 0
    # row starts
    assert got["rows"] == len(starts)
    assert np.array_equal(got["starts"], starts)
    tiles = -(-len(c["buf"]) // T.TILE)
    per_tile = np.bincount(starts // T.TILE, minlength=tiles)
    assert np.array_equal(got["tile_offsets"], np.cumsum(per_tile) - per_tile)  # the exclusive scan
    # the raw matrix, flagged rows included
    nan_g, nan_t = np.isnan(got["X_raw"]), np.isnan(X)
    assert np.array_equal(nan_g, nan_t), np.argwhere(nan_g != nan_t)[:5]
    assert np.array_equal(T.bits(got["X_raw"])[~nan_g], T.bits(X)[~nan_t])
    # flags
    k, cap = got["n_flagged"], c["max_flagged"]
    assert k == len(flagged)
    listed = got["flag_list"][: min(k, cap)]
    assert len(set(listed.tolist())) == len(listed) and set(listed.tolist()) <= set(flagged.tolist())
    if k <= cap:
        assert np.array_equal(np.sort(listed), flagged)
    assert (got["flag_list"][min(k, cap):] == T.SENTINEL32).all()  # slots past the count stay unwritten
    # guards
    for what, g in got["guards"].items():
        assert len(g) == T.GUARD and (g == (T.SENTINEL64 if what == "starts" else T.SENTINEL32)).all(), what
    print(f"{name}: {len(starts)} rows, {k} flagged, {len(c['buf'])} bytes")


def test_nine_missing_tokens_are_refused(gpu, lib):
    """``n_missing`` beyond the device table: -2 before any launch, nothing written."""
    c = T.case_named("capacity-64")
    got = _run(lib, gpu, c, missing=tuple(f"m{i}" for i in range(9)))
    assert got["rc"] == -2 and got["rows"] == 300
    assert (got["X_raw"].view(np.uint32) == T.SENTINEL32).all() and got["n_flagged"] == 0
    assert (got["flag_list"] == T.SENTINEL32).all()
    assert _run(lib, gpu, c, missing=tuple(f"m{i}" for i in range(8)))["rc"] == 0


# --------------------------------------------------------------------------- the reader


def _read_device(path, case, gpu, chunk, max_flagged, zero_copy):
    import torch

    from flink_jpmml_amd.stream.device_text import DeviceTextReader

    r = DeviceTextReader(str(path), T.Fields(case["F"]), T.columns_of(case["colmap"]), 0, path.stat().st_size, gpu,
                         delimiter=case["delim"].decode(), chunk_bytes=chunk, max_flagged=max_flagged,
                         zero_copy=zero_copy)
    mats = [b.X for b in r]
    torch.cuda.synchronize()
    m = torch.cat(mats).cpu().numpy() if mats else np.zeros((0, case["F"]), np.float32)
    return m, r


def _reader_case(buf, case):
    c = dict(case, buf=buf, missing=T.DEFAULT_MISSING)
    starts = T.twin_row_starts(buf)
    _, flagged = T.twin_parse(buf, starts, c["n_cols"], c["colmap"], c["F"], c["delim"], c["missing"])
    return c, T.host_parse(c), starts[flagged]


def _flags_per_chunk(data: bytes, chunk: int, flagged_starts) -> list:
    """Flagged records in every chunk of ``DeviceTextReader._chunks`` (``chunk`` bytes, then on
    through the next newline)."""
    out, a, hi = [], 0, len(data)
    while a < hi:
        b = min(hi, a + chunk)
        if b < hi:
            nl = data.find(b"\n", b - 1)
            b = hi if nl < 0 else nl + 1
        out.append(int(((flagged_starts >= a) & (flagged_starts < b)).sum()))
        a = b
    return out


@pytest.fixture(scope="module")
def reader_files(tmp_path_factory):
    """(path, case, host matrix, starts of the twin's flagged rows) per file; files end without a
    newline."""
    from flink_jpmml_amd.stream.device_text import release_mapped

    d = tmp_path_factory.mktemp("text")
    out = {}
    shapes = T.case_named("shapes-comma")
    for name, buf, case in (("five-flags", T.capacity_buffer(), T.case_named("capacity-5")),
                            ("messy", T.messy_corpus(), shapes),
                            ("shapes", shapes["buf"], shapes),
                            ("257-columns", T.case_named("global-257-columns")["buf"], T.case_named("global-257-columns")),
                            ("two-columns-one-field", T.case_named("shapes-comma-two-columns-one-field")["buf"] * 40,
                             T.case_named("shapes-comma-two-columns-one-field"))):
        c, H, fs = _reader_case(buf, case)
        p = d / f"{name}.csv"
        p.write_bytes(buf[:-1])  # the last line without a newline
        out[name] = (p, c, H, fs)
    yield out
    release_mapped()


@pytest.mark.parametrize("zero_copy", [False, True])
@pytest.mark.parametrize("max_flagged", [4, 5, 6])
def test_reader_around_the_flag_capacity(gpu, reader_files, max_flagged, zero_copy):
    """One chunk holds all five flagged records (4: the whole chunk goes to the host parser; 5 and
    6: the five rows are patched); small chunks hold at most a few."""
    p, c, H, fs = reader_files["five-flags"]
    k, data = len(fs), p.read_bytes()
    assert k == 5
    per = {chunk: _flags_per_chunk(data, chunk, fs) for chunk in (1 << 10, 1 << 12, 1 << 26)}
    assert per[1 << 26] == [5] and max(per[1 << 10]) <= 2 and len(per[1 << 10]) >= 8
    for chunk in per:
        m, r = _read_device(p, c, gpu, chunk, max_flagged, zero_copy)
        assert T.same_matrix(m, H), (chunk, np.argwhere(T.bits(m) != T.bits(H))[:5])
        assert r.rows_flagged == k


@pytest.mark.parametrize("zero_copy", [False, True])
def test_reader_overflowing_chunks_on_the_messy_corpus(gpu, reader_files, zero_copy):
    """``max_flagged=1``: chunks with two or more flagged records take the whole-chunk branch,
    chunks with one or none the patch branch; both occur at the small chunk sizes."""
    p, c, H, fs = reader_files["messy"]
    k, data = len(fs), p.read_bytes()
    assert k > 500 and len(H) > 2000
    per = _flags_per_chunk(data, 1 << 8, fs)
    assert sum(n > 1 for n in per) >= 100 and per.count(1) >= 10 and per.count(0) >= 1
    for chunk in (1 << 8, 1 << 12, 1 << 26):
        m, r = _read_device(p, c, gpu, chunk, 1, zero_copy)
        assert T.same_matrix(m, H), (chunk, np.argwhere(T.bits(m) != T.bits(H))[:5])
        assert r.rows_flagged == k
    m, r = _read_device(p, c, gpu, 1 << 14, 1 << 16, zero_copy)  # no chunk overflows
    assert T.same_matrix(m, H) and r.rows_flagged == k


@pytest.mark.parametrize("name", ["shapes", "257-columns", "two-columns-one-field"])
def test_reader_files_equal_host(gpu, reader_files, name):
    p, c, H, fs = reader_files[name]
    k = len(fs)
    for zero_copy in (False, True):
        for chunk in (1 << 9, 1 << 26):
            m, r = _read_device(p, c, gpu, chunk, 1 << 16, zero_copy)
            assert T.same_matrix(m, H), (name, chunk, zero_copy)
            assert r.rows_flagged == k
