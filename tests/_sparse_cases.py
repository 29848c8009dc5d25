"""Shapes, row patterns and the host yardstick shared by ``test_sparse_batch.py`` (the kernel's
numpy twin) and ``test_gpu_sparse.py`` (the kernel).

The yardstick is ``pack_vectors_masked`` cast to fp32: the host densification the project already
trusts. The expand only moves bits, so everything compares as ``uint32`` views, no tolerance.

Widths: 1 and 3 (tile bases off 16 bytes: the 4-byte store path), 4 and 64 (16-byte path), 33
(odd pitch, aligned only on every fourth row block), 257 (R = 63: odd pitch, an R that never
divides m), 4096 (R = 4) and 16384 (R = 1, the widest input any plan accepts). R = 256 for
widths <= 64. Row counts sit on both sides of the 256-row workgroup tile.
"""

import numpy as np

PAIRS = [
    (1, 1), (1, 257), (1, 1000),
    (3, 1), (3, 255), (3, 257),
    (4, 256), (4, 257), (4, 1000),
    (33, 255), (33, 257), (33, 1000),
    (64, 1), (64, 256), (64, 1000),
    (257, 1), (257, 255), (257, 1000),
    (4096, 1), (4096, 257),
    (16384, 1), (16384, 255),
]
PATTERNS = ["empty", "full", "one_full_first", "one_full_last", "random5", "edge_columns", "specials"]
FILLS = [float("nan"), -1.5]

SPECIALS = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-40, 1.5], dtype=np.float32)  # 1e-40: subnormal


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_csr(F: int, m: int, pattern: str, seed: int = 0):
    """``(indptr int32, indices int32, values fp32)`` of an ``[m, F]`` batch with the pattern."""
    rng = np.random.default_rng(seed * 1000003 + F * 131 + m)
    mask = np.zeros((m, F), dtype=bool)
    if pattern == "full":
        mask[:] = True
    elif pattern == "one_full_first":
        mask[0] = True
    elif pattern == "one_full_last":
        mask[m - 1] = True
    elif pattern == "random5":
        mask = rng.random((m, F)) < 0.05
    elif pattern == "edge_columns":
        mask[0::2, 0] = True
        mask[1::2, F - 1] = True
    elif pattern == "specials":
        mask = rng.random((m, F)) < 0.5
        mask[0, 0] = True
    elif pattern != "empty":
        raise ValueError(pattern)
    rows, cols = np.nonzero(mask)  # row-major: columns ascend within a row
    indptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(mask.sum(axis=1), out=indptr[1:])
    if pattern == "specials":
        values = SPECIALS[np.arange(rows.size) % SPECIALS.size]
    else:
        values = rng.standard_normal(rows.size).astype(np.float32)
    return indptr, cols.astype(np.int32), np.ascontiguousarray(values, dtype=np.float32)


def vectors_of(indptr, indices, values, F: int):
    from flink_jpmml_amd import SparseVector

    return [SparseVector(F, indices[a:b], values[a:b].astype(np.float64))
            for a, b in zip(indptr[:-1].tolist(), indptr[1:].tolist())]


def expected(indptr, indices, values, F: int):
    """``{fill: fp32 matrix}`` for both fills, from one ``pack_vectors_masked`` of the rows as
    SparseVectors: NaN where absent, or the fill exactly there (a stored NaN stays)."""
    from flink_jpmml_amd.api.vectors import pack_vectors, pack_vectors_masked

    vs = vectors_of(indptr, indices, values, F)
    X, absent, ok = pack_vectors_masked(vs, F)
    assert ok.all() and np.array_equal(bits(X), bits(pack_vectors(vs, F)))
    X32 = X.astype(np.float32)
    return {"nan": X32, "fill": np.where(absent, np.float32(-1.5), X32)}, absent


def skewed_vectors(n: int, F: int, seed: int = 0, value_scale: float = 1.0):
    """``n`` SparseVectors of width ``F`` with fp32-exact values and skewed density: empty rows,
    thin rows, a few full rows, some stored NaNs — so micro-batch slices differ a lot in nnz."""
    from flink_jpmml_amd import SparseVector

    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        u = rng.random()
        k = 0 if u < 0.2 else (F if u > 0.93 else int(rng.integers(1, max(2, F // 4 + 1))))
        idx = np.sort(rng.choice(F, size=min(k, F), replace=False))
        val = (value_scale * rng.standard_normal(idx.size)).astype(np.float32).astype(np.float64)
        if idx.size and i % 11 == 0:
            val[0] = np.nan
        out.append(SparseVector(F, idx, val))
    return out
