// CSR -> dense expansion of a record slice (gfx950 / CDNA4, wave64).
//
// A SparseRecordBatch crosses PCIe as three arrays (indptr, indices, values) instead of an [m, F]
// matrix full of NaN. This kernel rebuilds the dense [m, F] fp32 tile the model kernels read:
//
//   out[r, c] = values[k]   if row r stores column c at position k
//             = fill        otherwise (NaN = PMML missing, or the caller's replace_nan)
//
// A stored NaN stays NaN under any fill: the kernel only moves bits.
//
// One 256-thread workgroup owns R consecutive rows and builds their dense image in LDS: fill,
// barrier, scatter, barrier, stream out. Every global element is written exactly once, by
// coalesced stores (16-byte ones where the tile base allows it); the element-granular scatter,
// uncoalesced by nature, stays inside the LDS. The entries of R consecutive rows are one contiguous
// CSR range: all threads stride over it with coalesced index / value loads and find each entry's
// row by binary search over the R + 1 staged indptr words, so one full row among empty ones costs
// what a uniform spread costs.
#include "common.h"
#include <atomic>

struct CsrExpandArgs {
  const int* indptr;     // [m + 1], rebased: indptr[0] == 0
  const int* indices;    // [nnz] column of each stored entry
  const float* values;   // [nnz]
  float* out;            // [m, F] row-major, pitch F
  int m, F;
  int nnz;               // entries in the slice: positions outside [0, nnz) are never read
  float fill;
};

constexpr int CSR_TB = 256;
// dense image per workgroup: half of the 160 KiB LDS less the indptr words, so two workgroups fit a CU
constexpr int CSR_TILE_BYTES = 64 * 1024;
constexpr int CSR_MAX_F = CSR_TILE_BYTES / 4;  // 16384: the widest input any plan accepts; then R = 1
constexpr int CSR_MAX_R = 256;
constexpr int CSR_MAX_LDS = CSR_TILE_BYTES + (CSR_MAX_R + 1) * 4 + 12;  // image + indptr words, 16-byte rounded
constexpr int CSR_MAX_DEVICES = 64;

static inline int csr_rows(int F) {
  const int r = CSR_TILE_BYTES / (4 * F);
  return r < 1 ? 1 : (r > CSR_MAX_R ? CSR_MAX_R : r);
}

__global__ __launch_bounds__(CSR_TB) void csr_expand_kernel(CsrExpandArgs a, int R) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);  // [nr, F]
  const int F = a.F;
  const int r0 = blockIdx.x * R;
  const int nr = min(R, a.m - r0);
  const int count = nr * F;  // <= CSR_TILE_BYTES / 4
  int* iptr = reinterpret_cast<int*>(smem + (((size_t)R * F * 4 + 15) & ~(size_t)15));  // [nr + 1]
  const int t = threadIdx.x;

  for (int i = t; i <= nr; i += CSR_TB) iptr[i] = min(max(a.indptr[r0 + i], 0), a.nnz);
  const float fill = a.fill;
  const int c4 = count >> 2;
  const float4 f4 = make_float4(fill, fill, fill, fill);
  for (int i = t; i < c4; i += CSR_TB) reinterpret_cast<float4*>(tile)[i] = f4;
  for (int i = 4 * c4 + t; i < count; i += CSR_TB) tile[i] = fill;
  __syncthreads();

  const int k1 = iptr[nr];
  for (int k = iptr[0] + t; k < k1; k += CSR_TB) {
    const int c = a.indices[k];
    const float v = a.values[k];
    // row = the last i in [0, nr) with iptr[i] <= k (empty rows share their start with the next)
    int lo = 0, hi = nr;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (iptr[mid] <= k) lo = mid; else hi = mid;
    }
    if ((unsigned)c < (unsigned)F) tile[lo * F + c] = v;  // lo < nr, c < F: inside this tile
  }
  __syncthreads();

  float* dst = a.out + (size_t)r0 * F;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    for (int i = t; i < c4; i += CSR_TB) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(tile)[i];
    for (int i = 4 * c4 + t; i < count; i += CSR_TB) dst[i] = tile[i];
  } else {
    for (int i = t; i < count; i += CSR_TB) dst[i] = tile[i];
  }
}

PMML_API int pmml_csr_expand_args_size() { return (int)sizeof(CsrExpandArgs); }

// Rows of one workgroup for width F (the numpy twin in ops/sparse.py mirrors this).
PMML_API int pmml_csr_expand_rows(int F) { return (F < 1 || F > CSR_MAX_F) ? 0 : csr_rows(F); }

PMML_API int pmml_csr_expand(hipStream_t stream, const CsrExpandArgs* args) {
  const CsrExpandArgs a = *args;
  if (a.m < 0 || a.nnz < 0 || a.F < 1 || a.F > CSR_MAX_F) return -1;
  if (a.m == 0) return 0;
  if (!a.indptr || !a.out || (a.nnz > 0 && (!a.indices || !a.values))) return -2;
  const int R = csr_rows(a.F);
  const size_t lds = (((size_t)R * a.F * 4 + 15) & ~(size_t)15) + (size_t)(R + 1) * 4;
  if (lds > 65536) {
    // once per device, for the largest request any width makes: not a runtime call per micro-batch
    static std::atomic<bool> raised[CSR_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -5;
    if (dev < 0 || dev >= CSR_MAX_DEVICES || !raised[dev].load(std::memory_order_acquire)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(csr_expand_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, CSR_MAX_LDS);
      if (e != hipSuccess) return (int)e;
      if (dev >= 0 && dev < CSR_MAX_DEVICES) raised[dev].store(true, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(csr_expand_kernel, dim3((a.m + R - 1) / R), dim3(CSR_TB), lds, stream, a, R);
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
