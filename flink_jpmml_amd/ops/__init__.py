"""Native HIP kernel library (``_pmml_kernels.so``, gfx950) and its ctypes ABI.

Kernels (``csrc/``): ``tree.hip`` (perfect / pointer / wide tree-ensemble traversal, split
reduce), ``cluster.hip`` (center-based clustering), ``linear.hip`` (regression tables + links),
``mlp.hip`` (fused all-layer MFMA MLP, bf16 and fp32), ``svm.hip`` (kernel eval + votes),
``sparse.hip`` (CSR record batches expanded into the dense input tile; wrapper and numpy twin in
``sparse.py``), ``outputs.hip`` (Output fields and top-k classes; ``outputs.py``), ``reasons.hip``
(ranked Scorecard reason codes; wrapper, packed tables and numpy twin in ``reasons.py``),
``entities.hip`` (ranked entity ids and affinities of the clustering and k-NN families; wrapper,
tables and numpy twin in ``entities.py``), ``host.hip`` (zero-copy / copy helpers). Shared device
code: ``common.h`` (field preparation, LDS staging), ``epilogue.h`` (fused target decode),
``distance.h`` (per-field comparison, raw sums and the register top-k of ``knn.hip`` / ``entities.hip``).
"""

from ._lib import KernelLibraryError, LIB_PATH, build, host_device_ptr, is_stale, load

__all__ = ["KernelLibraryError", "LIB_PATH", "build", "host_device_ptr", "is_stale", "load"]
