// Wide regression tables on the matrix cores: y_k = b_k + Σ_f W[f][k]·x_f for up to 256 tables and
// 1024 fields, then the epilogue of linear.hip (simplemax division, apply_epilogue<true>).
// linear.hip keeps one lane per row and 16 register accumulators; past 16 tables x 128 fields the
// same product is a GEMM, run here on the exact-fp32 v_mfma_f32_32x32x2_f32.
//
// Workgroup: 256 threads (4 waves), a tile of 64 rows, K padded to Kp (a multiple of 32).
//   * Tables lie on the MFMA's M (accumulator registers), rows on its N (lanes 0-31), so a lane's
//     16 results are 16 tables of ONE row and go to LDS as acc[k][row] with consecutive lanes on
//     consecutive banks.
//   * Wave w owns the 32-row block (w & 1) and the table blocks (w >> 1), (w >> 1) + 2, ...: at most
//     4 accumulators = 64 registers, one X operand read per 4 MFMAs. (The issue's sketch gave a wave
//     both row blocks and every 4th table block; with few tables that leaves three waves without
//     an MFMA, this split keeps two busy from one table block on.)
//   * The K-loop runs over slices of 32 fields, double-buffered: the next slice's X quad loads
//     (16 bytes when ldx % 4 == 0 and the base is aligned, else scalar) and W float4 loads are in
//     flight while the MFMAs of the current slice run, then go to the other LDS buffer; one barrier
//     per slice. X passes through prep_value on its way into LDS (no prepare pass), which also
//     records per row: preparation rejected, NaN after preparation, ±inf after preparation.
//   * LDS layouts, both free of bank conflicts for the 64-lane operand reads (lanes 32-63 read the
//     next field): X slice [32 fields][64 rows] with the row index of odd fields XOR 32; W slice
//     [32 fields][Ks], Ks = Kp or Kp + 32, whichever is 32 mod 64.
//   * ±inf: a dense product would form 0·inf = NaN in every table that does not list the field (the
//     packed W holds 0 there; the oracle and linear.hip never form that product). The staging puts 0
//     into the operand and flags the row; the lane that finishes a flagged row re-reads the row and
//     adds the infinite terms in field order to the listed tables only (listed[F][Kp/32] words,
//     NULL: every table lists every field). An explicit coefficient of 0 is listed: 0·inf voids
//     the row, as in the oracle. Rows without an infinity never take this path.
//   * Finish: the accumulators (started on the bias) go to LDS over the staging buffers as
//     acc[k][72-row stride]; after one barrier lane r < 64 finishes row r exactly as linear.hip does.
#include "epilogue.h"

namespace {

constexpr int TB = 256;
constexpr int RT = 64;    // rows per workgroup
constexpr int FS = 32;    // fields per slice
constexpr int AS = 72;    // row stride of the finished accumulators: lanes 32-63 (table + 4) land 32 banks on
constexpr int KMAX = 256;
constexpr int FMAX = 1024;

enum : int { ROW_BAD = 1, ROW_MISS = 2, ROW_INF = 4 };

struct LinearWideArgs {
  const float* X;
  int n_rows, n_feat, ldx, K;
  const FieldPrep* prep;
  const float* W;      // [Fp][Kp], zero padded
  const float* bias;   // [Kp], zero padded
  int Kp, Fp;
  int simplemax, pad;
  Epilogue epi;
  float* score;
  uint8_t* valid;
  float* probs;
  const uint32_t* listed;  // [F][Kp / 32] bit k: table k lists predictor f; NULL: all listed
};

typedef float f32x16_t __attribute__((ext_vector_type(16)));

// raw X of one slice into registers. Quad path: thread = (row e & 63, field quad e >> 6), two quads;
// scalar path: thread = (row e >> 5, field e & 31), eight values. Out of range: 0.
__device__ __forceinline__ void load_x(const LinearWideArgs& a, bool quads, int row0, int f0, float (&xr)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) xr[j] = 0.f;
  if (quads) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = threadIdx.x + TB * j;
      const int row = row0 + (e & 63), f = f0 + 4 * (e >> 6);
      if (row < a.n_rows && f < a.n_feat) {  // the last quad may read past F, inside the row's stride
        const float4 v = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + f);
        xr[4 * j] = v.x, xr[4 * j + 1] = v.y, xr[4 * j + 2] = v.z, xr[4 * j + 3] = v.w;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = threadIdx.x + TB * j;
      const int row = row0 + (e >> 5), f = f0 + (e & 31);
      if (row < a.n_rows && f < a.n_feat) xr[j] = a.X[(size_t)row * a.ldx + f];
    }
  }
}

// one prepared value for the MFMA operand, the row's flags in *fl
__device__ __forceinline__ float operand(const LinearWideArgs& a, float x, int f, int* fl) {
  bool b = false;
  if (a.prep) x = prep_value(x, a.prep[f], &b);
  if (b) *fl |= ROW_BAD;
  if (x != x) *fl |= ROW_MISS;
  if (__builtin_isinf(x)) {
    *fl |= ROW_INF;
    x = 0.f;
  }
  return x;
}

__device__ __forceinline__ void store_x(const LinearWideArgs& a, bool quads, int row0, int f0, const float (&xr)[8],
                                        float* __restrict__ xs, int* __restrict__ flags) {
  if (quads) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = threadIdx.x + TB * j;
      const int r = e & 63, q = e >> 6;
      const bool in = row0 + r < a.n_rows;
      int fl = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int s = 4 * q + k;
        float x = xr[4 * j + k];
        x = (in && f0 + s < a.n_feat) ? operand(a, x, f0 + s, &fl) : 0.f;
        xs[s * RT + (r ^ ((s & 1) << 5))] = x;
      }
      if (fl) atomicOr(&flags[r], fl);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = threadIdx.x + TB * j;
      const int r = e >> 5, s = e & 31;
      int fl = 0;
      float x = xr[j];
      x = (row0 + r < a.n_rows && f0 + s < a.n_feat) ? operand(a, x, f0 + s, &fl) : 0.f;
      xs[s * RT + (r ^ ((s & 1) << 5))] = x;
      if (fl) atomicOr(&flags[r], fl);
    }
  }
}

// the W slice [32][Kp] is contiguous in the packed matrix: ncb float4 per thread
__device__ __forceinline__ void load_w(const LinearWideArgs& a, int ncb, int f0, float4 (&wr)[8]) {
  const float4* src = reinterpret_cast<const float4*>(a.W + (size_t)f0 * a.Kp);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    wr[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < ncb) wr[j] = src[threadIdx.x + TB * j];
  }
}

__device__ __forceinline__ void store_w(const LinearWideArgs& a, int ncb, int Ks, const float4 (&wr)[8],
                                        float* __restrict__ ws) {
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < ncb) {
      const int q = 4 * (threadIdx.x + TB * j);
      const int f = q / a.Kp, c = q - f * a.Kp;
      *reinterpret_cast<float4*>(ws + f * Ks + c) = wr[j];
    }
}

__global__ __launch_bounds__(TB) void linear_wide_kernel(LinearWideArgs a, int Ks) {
  extern __shared__ __align__(16) float lds[];
  // [xs0 | xs1 | ws0 | ws1 | flags]; the finished accumulators reuse it from the start
  float* xs = lds;
  float* ws = lds + 2 * FS * RT;
  int* flags = reinterpret_cast<int*>(ws + 2 * FS * Ks);
  float* accs = lds;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int row0 = blockIdx.x * RT;
  const int ncb = a.Kp >> 5;
  const int rb = wave & 1, cb0 = wave >> 1;
  const int nj = cb0 < ncb ? (ncb - cb0 + 1) >> 1 : 0;  // this wave's table blocks cb0, cb0 + 2, ...
  const bool quads = (a.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15) == 0;
  const int n_slices = (a.n_feat + FS - 1) / FS;

  if (tid < RT) flags[tid] = 0;
  f32x16_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      acc[j][i] = j < nj ? a.bias[(cb0 + 2 * j) * 32 + (i & 3) + 8 * (i >> 2) + 4 * half] : 0.f;

  float xr[8];
  float4 wr[8];
  load_x(a, quads, row0, 0, xr);
  load_w(a, ncb, 0, wr);
  __syncthreads();  // flags cleared
  store_x(a, quads, row0, 0, xr, xs, flags);
  store_w(a, ncb, Ks, wr, ws);
  __syncthreads();

  for (int s = 0; s < n_slices; ++s) {
    const bool more = s + 1 < n_slices;
    if (more) {
      load_x(a, quads, row0, (s + 1) * FS, xr);
      load_w(a, ncb, (s + 1) * FS, wr);
    }
    const float* xb = xs + (s & 1) * FS * RT;
    const float* wb = ws + (s & 1) * FS * Ks;
#pragma unroll 4
    for (int kk = 0; kk < FS / 2; ++kk) {
      const int f = 2 * kk + half;  // f & 1 == half
      const float x = xb[f * RT + ((rb * 32 + l31) ^ (half << 5))];
      const float* wrow = wb + f * Ks + cb0 * 32 + l31;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nj) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[64 * j], x, acc[j], 0, 0, 0);
    }
    if (more) {  // the other buffer was last read before the previous barrier
      store_x(a, quads, row0, (s + 1) * FS, xr, xs + ((s + 1) & 1) * FS * RT, flags);
      store_w(a, ncb, Ks, wr, ws + ((s + 1) & 1) * FS * Ks);
    }
    __syncthreads();
  }

  // every operand read is behind the last barrier; the accumulators overwrite the staging buffers
  // and end before the flags (Kp x 72 <= 4096 + 64 Ks)
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nj) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {  // D[table (i&3) + 8(i>>2) + 4 half][row lane & 31]
        const int k = (cb0 + 2 * j) * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
        accs[k * AS + rb * 32 + l31] = acc[j][i];
      }
    }
  __syncthreads();

  const int row = row0 + tid;
  if (tid >= RT || row >= a.n_rows) return;
  float* mine = accs + tid;
  const int fl = flags[tid];
  if (fl & ROW_INF) {
    const int words = a.Kp >> 5;
    for (int f = 0; f < a.n_feat; ++f) {
      float x = a.X[(size_t)row * a.ldx + f];
      bool b = false;
      if (a.prep) x = prep_value(x, a.prep[f], &b);
      if (!__builtin_isinf(x)) continue;
      for (int k = 0; k < a.K; ++k) {
        const bool on = !a.listed || ((a.listed[(size_t)f * words + (k >> 5)] >> (k & 31)) & 1u);
        if (on) mine[k * AS] = fmaf(a.W[(size_t)f * a.Kp + k], x, mine[k * AS]);
      }
    }
  }
  if (a.simplemax) {
    float s = 0.f;
    for (int k = 0; k < a.K; ++k) s += mine[k * AS];
    for (int k = 0; k < a.K; ++k) mine[k * AS] /= s;
  }
  apply_epilogue<true>(a.epi, [&](int c) { return mine[c * AS]; }, !(fl & (ROW_BAD | ROW_MISS)), row, a.n_rows,
                       a.score, a.valid, a.probs);
}

}  // namespace

PMML_API int pmml_linear_wide_args_size() { return (int)sizeof(LinearWideArgs); }

PMML_API int pmml_linear_wide_launch(hipStream_t stream, const LinearWideArgs* args) {
  const LinearWideArgs a = *args;
  if (a.K > KMAX || a.n_feat > FMAX || a.K < 1 || a.n_feat < 1) return -4;
  if ((a.Kp & 31) || a.Kp < a.K || a.Kp > KMAX || (a.Fp & (FS - 1)) || a.Fp < a.n_feat || a.ldx < a.n_feat)
    return -4;
  if (a.epi.mode != EPI_AFFINE && a.epi.n_classes > a.K) return -4;
  if (a.n_rows <= 0) return 0;
  const int Ks = (a.Kp & 63) == 32 ? a.Kp : a.Kp + 32;
  // staging 2 (32 x 64 + 32 Ks) floats; the accumulators Kp x 72 fit inside it (8 Kp <= 4096)
  const size_t lds = (size_t)(2 * FS * RT + 2 * FS * Ks + RT) * 4;
  dim3 grid((a.n_rows + RT - 1) / RT);
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(linear_wide_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -5;
  hipLaunchKernelGGL(linear_wide_kernel, grid, dim3(TB), lds, stream, a, Ks);
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
