"""CSR → dense expansion on the device (``csrc/sparse.hip``) and its numpy twin.

``csr_expand`` launches ``pmml_csr_expand``: ``out[r, c] = values[k]`` where row ``r`` stores
column ``c`` at position ``k``, else ``fill`` (NaN = PMML missing, or the caller's
``replace_nan``). A stored NaN stays NaN under any fill.

``csr_expand_numpy`` walks the same tiles with the same row search and the same defensive bounds
on the host; the CPU tests pin it to :func:`flink_jpmml_amd.api.vectors.pack_vectors`.
"""

from __future__ import annotations

import numpy as np

TILE_BYTES = 64 * 1024  # dense image of one workgroup: half the 160 KiB LDS less the indptr words
MAX_WIDTH = TILE_BYTES // 4  # 16384, the widest input any plan accepts; a wider batch densifies on the host
MAX_ROWS = 256
THREADS = 256


def rows_per_block(width: int) -> int:
    """``R``: consecutive rows one workgroup stages in LDS (``sparse.hip`` ``csr_rows``)."""
    if not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"csr_expand handles 1 <= width <= {MAX_WIDTH}, got {width}")
    return max(1, min(MAX_ROWS, TILE_BYTES // (4 * width)))


def csr_expand(indptr, indices, values, out, nnz: int, fill: float = float("nan"), stream=None) -> None:
    """Expand the CSR slice (device tensors: ``indptr`` int32 ``[m+1]`` rebased to 0, ``indices``
    int32 and ``values`` float32 with at least ``nnz`` entries) into the contiguous device tensor
    ``out`` ``[m, F]`` float32 on ``stream``."""
    from . import _lib

    m, F = int(out.shape[0]), int(out.shape[1])
    if not out.is_contiguous() or int(indptr.numel()) < m + 1:
        raise ValueError("csr_expand needs a contiguous [m, F] output and m + 1 indptr words")
    if int(indices.numel()) < nnz or int(values.numel()) < nnz:
        raise ValueError(f"csr_expand: {nnz} entries announced, buffers hold fewer")
    rows_per_block(F)
    a = _lib.CsrExpandArgs()
    a.indptr, a.indices, a.values, a.out = indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), out.data_ptr()
    a.m, a.F, a.nnz, a.fill = m, F, int(nnz), float(fill)
    _lib.check(_lib.load().pmml_csr_expand(_lib.stream_handle(stream), a), "pmml_csr_expand")


def csr_expand_numpy(indptr: np.ndarray, indices: np.ndarray, values: np.ndarray, m: int, width: int,
                     fill: float = float("nan")) -> np.ndarray:
    """The kernel on the host, tile by tile: fill the ``R × width`` image, scatter the tile's
    contiguous entry range with each entry's row found by binary search over the tile's ``R + 1``
    indptr words, skip what falls outside (``index >= width``, positions outside the slice)."""
    R = rows_per_block(width)
    nnz = int(min(len(indices), len(values)))
    indptr = np.asarray(indptr, dtype=np.int64)
    out = np.empty((m, width), dtype=np.float32)
    for r0 in range(0, m, R):
        nr = min(R, m - r0)
        iptr = np.clip(indptr[r0:r0 + nr + 1], 0, nnz)
        tile = np.full(nr * width, fill, dtype=np.float32)
        k = np.arange(iptr[0], iptr[nr])
        if k.size:
            # the last i in [0, nr) with iptr[i] <= k, as the kernel's search finds it
            lo = np.zeros(k.size, dtype=np.int64)
            hi = np.full(k.size, nr, dtype=np.int64)
            while True:
                live = hi - lo > 1
                if not live.any():
                    break
                mid = (lo + hi) >> 1
                down = live & (iptr[np.minimum(mid, nr)] <= k)
                lo = np.where(down, mid, lo)
                hi = np.where(live & ~down, mid, hi)
            c = np.asarray(indices[k], dtype=np.int64)
            ok = (c >= 0) & (c < width)
            tile[lo[ok] * width + c[ok]] = np.asarray(values[k], dtype=np.float32)[ok]
        out[r0:r0 + nr] = tile.reshape(nr, width)
    return out


__all__ = ["MAX_WIDTH", "csr_expand", "csr_expand_numpy", "rows_per_block"]
